"""Directed work lists for the intra pass (builders only: no GPU, no reference).

The random generator (openhevc_amd/synth/synth.c) takes every block's candidate flags from what was recorded before it, draws
modes and sizes independently of the position and never meets a threshold on purpose.  The families below enumerate what it
cannot reach.  Every list is recorded through the recorder's C ABI (oh_rec_begin / oh_rec_tu / oh_rec_intra / oh_rec_finish) with
the in-loop filters off, and keeps this contract, asserted by check_contract() on every list that is built:

  1  the schedule (levels, sub-levels) is the recorder's, never written by hand;
  2  a flag is set only if the neighbour precedes the block in decode (z-scan, 6.4.1) order and lies inside the picture
     (zscan_avail); any subset of those flags is legal (a neighbour in another slice or tile is unavailable);
  3  no sample a block reads is written by a block recorded later;
  4  a block that reads another recorded block is recorded after it and follows it in decode order.

  F  flags x mode x size x plane          build_f(chroma, bd, part)
  G  picture edges                        build_g(chroma, bd, what)
  H  thresholds                           build_h_thr(bd, variant, ...), build_h_clip(bd)
  J  occupancy and chains                 build_j(chroma, bd)
  K  constrained intra prediction         build_k8(...), build_k_big(chroma, bd), build_k_edge(chroma, bd)

Placement: a block of N x N luma samples (for chroma: the luma rectangle it covers) is the top-left quarter of a 2N x 2N cell
aligned to 2N at x, y >= 2N; the five neighbour runs then precede it in z-scan and lie in untouched quarters of other cells (K
and the clip lists of H use 4N cells, so that neighbouring blocks' map cells / constructed edges do not meet).

Counts (blocks / pictures), as printed by tests/test_directed_intra_lists.py -s:
  F  4:2:0 8 bit 7840 / 189, 10 bit 7840 / 194 (19 parts each); 4:2:0 12 bit 7072 / 103 (11 parts); 4:2:2 10 bit 7072 + 3360
     lower halves / 100 (10 parts); 4:4:4 8 bit 7424 / 96, 12 bit 7424 / 95 (10 parts each); mono 8 bit 3712 / 94 (9 parts)
  G  4:2:0 8 bit 1386 / 243, 4:4:4 10 bit 1638 / 261, 4:2:2 10 bit 1338 / 193: up-right and bottom-left runs cut at every multiple
     of 4 the plane's size allows (multiples of 8 in a plane that is not subsampled: pictures are multiples of 8 wide and high),
     18 (mode, flags) pairs each; x = 0 / y = 0 blocks with every subset x G_MODES; the 8x8 / 16x8 / 8x16 pictures
  H  per bit depth 2 sign pairs x 4 flag sets x 9 (t, l) pairs = 72 blocks in 8 pictures of 448x448, the same with strong smoothing
     off and with smoothing disabled, in a 4:4:4 chroma plane and (16x16) in a 4:2:0 chroma plane; 72 clip blocks in 4 pictures
  J  per format 3 CTU sizes x (one CTU, a row of four, 3 x 3) x 2 seeds = 18 pictures: 4602 blocks (4:2:0 8 bit), 8721 (4:4:4 10 bit)
  K  8x8: 512 masks with all flags + 3 x 128 with other flag sets = 896 blocks / 28 pictures, 224 / 8 with 8x8 min PUs; larger and
     chroma blocks 502 / 46 and 45; picture edge 294 / 42 per format

Counter totals of the oracle over the lists (oracle.h: OH_CNT_I_*, CPU), per family and format, so that a change that empties a
branch shows in review.  F (format = chroma_format_idc, bit depth): substitution from left / up-left / up / up-right / nothing,
smoothing 3-tap / strong, mode 10 clip low / high, mode 26 clip low / high, projected side samples:
  F 1  8    1960 /  980 / 490 / 245 / 245    1883 / 165    21 / 27    51 / 26    2848
  F 1 10    1960 /  980 / 490 / 245 / 245    1875 / 173    30 /  9    11 / 15    2848
  F 1 12    1768 /  884 / 442 / 221 / 221    1234 /  46    14 / 20    50 / 36    2464
  F 2 10    2608 / 1304 / 862 / 221 / 221    1246 /  34    20 / 35    37 / 22    3648
  F 3  8    1856 /  928 / 464 / 232 / 232    2533 /  27    20 / 22    81 / 47    2560
  F 3 12    1856 /  928 / 464 / 232 / 232    2536 /  24    19 / 33    30 / 59    2560
  F 0  8     928 /  464 / 232 / 116 / 116    1248 /  32    19 / 28    26 / 62    1280
G: tr partial / bl partial, substitution from nothing / up / up-right, projected, smoothing 3-tap / strong:
  G 1  8    216 / 216    333 / 318 /  90    459    223 / 24
  G 3 10    216 / 216    387 / 378 / 108    540    711 / 34
  G 2 10    216 / 108    333 / 366 /  90    443    225 / 24
H, the same at 8, 10 and 12 bit: (t < lim, l < lim) outcomes yes-yes / yes-no / no-yes / no-no, smoothing strong / 3-tap / none:
  strong smoothing on     8 / 16 / 16 / 32     8 / 64 /  0
  strong smoothing off    8 / 16 / 16 / 32     0 / 72 /  0
  smoothing disabled      0 /  0 /  0 /  0     0 /  0 / 72
  4:4:4 chroma plane      -                    0 / 72 /  0
  4:2:0 chroma plane      -                    0 /  0 / 72
  clip lists              mode 10 and mode 26 each: low 28, high 28, in range 168; DC edge filter 24
J: substitution from left / up / nothing, smoothing 3-tap / strong, mode 10 clip low / high, mode 26 clip low / high, projected:
  J 1  8    3062 / 245 / 54    232 / 22    153 / 109    128 / 138     774
  J 3 10    5808 / 285 / 54    741 / 12    102 / 134    129 / 178    1455
K: top-row search without left flags / x = 0 zero fill / up sweep / corner patch / flags cleared:
  K 8x8, 4x4 min PUs     112 /  0 / 848 / 400 / 1792
  K 8x8, 8x8 min PUs      36 /  0 / 180 /  84 /  528
  K large 1  8            27 /  0 / 473 / 217 /  823
  K large 3 10            36 /  0 / 463 / 212 /  948
  K edge 1  8             99 / 99 /  95 /   0 /  120
  K edge 3 10             94 / 94 / 100 /   0 /  135
  The start from the top row WITH a left flag is 0 in all of them and cannot be more with realisable flags: a left-side flag
  survives the re-derivation only if a cell of its run is intra, and a block off the min-PU grid has its own PU there.
"""
import functools

import numpy as np

import directed as D
from openhevc_amd import frame as F

BL, L, UL, U, UR = F.AV_BOTTOM_LEFT, F.AV_LEFT, F.AV_UP_LEFT, F.AV_UP, F.AV_UP_RIGHT
ALL5 = BL | L | UL | U | UR
MAX_DIM = D.MAX_DIM

F_FULL = [(1, 8), (1, 10)]                                    # (chroma_format_idc, bit depth): the full matrix
F_CUT = [(1, 12), (2, 10), (3, 8), (3, 12), (0, 8)]           # sizes <= 16 in full, 32x32 with CUT_MODES_32
CUT_MODES_32 = (0, 1, 2, 9, 10, 11, 18, 25, 26, 27, 34)
# residual kinds (make_res) the matrix cycles through by index.  A DC coefficient of +-32767 drives the whole block to the maximum or
# to 0 whatever was predicted: such a block checks the add and its clip, not the prediction.  The cycle is shifted by the format's
# index, and no two neighbours in it saturate, so every triple that two or more formats hold shows its prediction in one of them
# (tests/test_directed_intra_lists.py: test_every_triple_shows_its_prediction_in_some_format)
F_KINDS = (0, 1, 2, 0, 1, 3)
F_PARTS = {(1, 8): 19, (1, 10): 19, (1, 12): 11, (2, 10): 10, (3, 8): 10, (3, 12): 10, (0, 8): 9}
G_FORMATS = [(1, 8), (3, 10), (2, 10)]
G_MODES = (0, 1, 2, 10, 18, 26, 34, 14, 22)                   # 14 / 22: a negative angle on each side
G_KINDS = ("tr", "bl", "origin", "tiny")
H_DEPTHS = (8, 10, 12)
H_FLAGS = (ALL5, ALL5 & ~UR, ALL5 & ~BL, ALL5 & ~(UR | BL))
H_SIGNS = ((1, -1), (-1, 1))
H_MODES = (0, 2, 18, 34, 9, 27, 11, 25, 3)                    # 32x32: every mode but 1, 10, 26 smooths
J_FORMATS = [(1, 8), (3, 10)]
J_MODES = (2, 18, 34, 10, 26, 0)
J_OCCUPANCY = (1, 2, 3, 4, 5, 8, 9)
K_FORMATS = [(1, 8), (3, 10)]
K_MODES = (0, 1, 10, 26, 2, 34)
K_SUBSETS = (UL | U | UR, BL | L, L | UL | U)


def chroma_sizes(chroma):
    """log2 sizes of chroma blocks: 4:2:0 and 4:2:2 halve the transform unit's width, 4x4 is the smallest"""
    return {0: (), 1: (2, 3, 4), 2: (2, 3, 4), 3: (2, 3, 4, 5)}[chroma]


def flag_names(a):
    return "+".join(n for b, n in ((BL, "bottom-left"), (L, "left"), (UL, "up-left"), (U, "up"), (UR, "up-right")) if a & b) or "none"


# -------------------------------------------------------------------------------------------------------------- records ----
class Blk:
    """one recorded intra block (position in samples of plane c) and what it was chosen for"""
    __slots__ = ("c", "x", "y", "log2", "mode", "avail", "tu", "note", "lower", "cell", "cx", "cy", "mask", "edge", "tag")

    def __init__(self, c, log2, mode, avail, tu=None, note="", x=0, y=0):
        self.c, self.x, self.y, self.log2, self.mode, self.avail, self.tu, self.note = c, x, y, log2, mode, avail, tu, note
        self.lower = self.mask = self.edge = self.tag = None
        self.cell = self.cx = self.cy = 0

    @property
    def n(self):
        return 1 << self.log2

    def __repr__(self):
        return (f"intra {self.n}x{self.n} plane {self.c} at ({self.x}, {self.y}) mode {self.mode} flags {self.avail:05b} ({flag_names(self.avail)}) "
                f"residual: {self.tu.recipe if self.tu is not None else 'none'} {self.note}")


class IntraList(D.DirectedList):
    """a recorded list of intra blocks; `patches` are samples constructed into the current picture's initial content"""
    blks, patches, is_intra = (), (), None

    def pictures(self):
        pics = super().pictures()
        for c, x, y, a in self.patches:
            a = np.atleast_2d(a)
            pics[2].planes[c][y:y + a.shape[0], x:x + a.shape[1]] = a
        return pics

    def item_at(self, c, x, y):
        hit = [repr(b) for b in self.blks if b.c == c and b.x <= x < b.x + b.n and b.y <= y < b.y + b.n]
        return "; ".join(hit) if hit else "no item (initial content)"


def params(width, height, chroma, bd, **kw):
    return F.pic_params(width, height, bit_depth=bd, chroma_format_idc=chroma, sao=0, deblock=0, transquant_bypass_enable=1, **kw)


def make_res(rng, kind, log2, c, bd):
    """0 none, 1 a small random residual, 2 / 3 a DC coefficient of +-32767 (the clip after the add acts), 4 / 5 the whole block
    driven to the maximum / to 0 (bypass residual of +-2^bd)"""
    n = 1 << log2
    if kind == 0:
        return None
    if kind == 1:
        co = rng.integers(-64, 65, size=(n, n)) * (rng.random((n, n)) < 0.15)
        co[0, 0] = int(rng.integers(-200, 201))
        return D.Tu(log2, F.TU_IDCT, 0, co, "small random", c=c, intra=True)
    if kind in (2, 3):
        co = np.zeros((n, n), np.int16)
        co[0, 0] = 32767 if kind == 2 else -32767
        return D.Tu(log2, F.TU_IDCT, 0, co, f"DC coefficient {co[0, 0]}", c=c, intra=True)
    v = (1 << bd) if kind == 4 else -(1 << bd)
    return D.Tu(log2, F.TU_BYPASS, 0, np.full((n, n), v, np.int16), f"bypass residual {v}: block driven to {'the maximum' if v > 0 else '0'}", c=c, intra=True)


# ------------------------------------------------------------------------------------------------- z-scan availability ----
def _zaddr(p, X, Y):
    """decode-order address of the 4x4 luma unit that holds luma sample (X, Y): CTB raster, Morton inside the CTB"""
    lc = p.log2_ctb_size
    ctbw = (p.width + (1 << lc) - 1) >> lc
    xi, yi = (X & ((1 << lc) - 1)) >> 2, (Y & ((1 << lc) - 1)) >> 2
    m = 0
    for b in range(4):
        m |= ((xi >> b) & 1) << (2 * b) | ((yi >> b) & 1) << (2 * b + 1)
    return (((Y >> lc) * ctbw + (X >> lc)) << 8) | m


def luma_rect(p, c, x, y, n):
    hs, vs = F.hshift(p, c), F.vshift(p, c)
    return x << hs, y << vs, n << hs, n << vs


def zscan_avail(p, c, x, y, n):
    """the candidate flags a decoder can give the n x n block at (x, y) of plane c at most: a neighbour run counts if the part of it
    inside the picture is not empty and every 4-sample unit of that part precedes the block in decode order (6.4.1)"""
    X0, Y0, nh, nv = luma_rect(p, c, x, y, n)
    cur = _zaddr(p, X0, Y0)

    def run(pts):
        pts = [(X, Y) for X, Y in pts if 0 <= X < p.width and 0 <= Y < p.height]
        return bool(pts) and all(_zaddr(p, X, Y) < cur for X, Y in pts)
    a = 0
    if run([(X0 - 1, Y0 - 1)]):
        a |= UL
    if run([(X0 + i, Y0 - 1) for i in range(0, nh, 4)]) and Y0 > 0:
        a |= U
    if Y0 > 0 and run([(X0 + nh + i, Y0 - 1) for i in range(0, nh, 4)]):
        a |= UR
    if X0 > 0 and run([(X0 - 1, Y0 + i) for i in range(0, nv, 4)]):
        a |= L
    if X0 > 0 and run([(X0 - 1, Y0 + nv + i) for i in range(0, nv, 4)]):
        a |= BL
    return a


def decode_key(p, b):
    """decode order of a block: CTB raster, Morton order of its luma position inside the CTB, plane; the 4x4 chroma blocks of an 8x8
    4:2:0 unit follow its fourth luma block (hevc.c:1395)"""
    X0, Y0, _, _ = luma_rect(p, b.c, b.x, b.y, b.n)
    if b.c and p.chroma_format_idc == 1 and b.log2 == 2:
        X0, Y0 = X0 + 4, Y0 + 4
    return (_zaddr(p, X0, Y0), b.c)


def read_regions(p, b):
    """[(rows, columns)] slices of plane b.c the block gathers with its flags (hevcpred_template.c:164-183)"""
    pw, ph = F.plane_dims(p, b.c)
    x, y, n, out = b.x, b.y, b.n, []
    if b.avail & UL:
        out.append((slice(y - 1, y), slice(x - 1, x)))
    if b.avail & U:
        out.append((slice(y - 1, y), slice(x, x + n)))
    if b.avail & UR:
        out.append((slice(y - 1, y), slice(x + n, min(x + 2 * n, pw))))
    if b.avail & L:
        out.append((slice(y, y + n), slice(x - 1, x)))
    if b.avail & BL:
        out.append((slice(y + n, min(y + 2 * n, ph)), slice(x - 1, x)))
    return out


def check_contract(dl):
    """items 2-4 of the contract and no two blocks overlapping; raises AssertionError naming the block"""
    p = dl.p
    widx = [np.full(F.plane_dims(p, c)[::-1], -1, np.int32) for c in range(F.n_planes(p))]
    for i, b in enumerate(dl.blks):
        pw, ph = F.plane_dims(p, b.c)
        assert 0 <= b.x and 0 <= b.y and b.x + b.n <= pw and b.y + b.n <= ph, (dl.name, b)
        w = widx[b.c][b.y:b.y + b.n, b.x:b.x + b.n]
        assert (w == -1).all(), f"{dl.name}: {b} overlaps {dl.blks[int(w.max())]}"
        w[:] = i
    keys = [decode_key(p, b) for b in dl.blks]
    for i, b in enumerate(dl.blks):
        real = zscan_avail(p, b.c, b.x, b.y, b.n)
        assert not b.avail & ~real, f"{dl.name}: {b} has flags no decoder gives it (realisable: {flag_names(real)})"
        for rows, cols in read_regions(p, b):
            w = widx[b.c][rows, cols]
            assert w.size and (w < i).all(), f"{dl.name}: {b} reads samples of a block recorded later"
            for j in np.unique(w[w >= 0]):
                assert keys[int(j)] < keys[i], f"{dl.name}: {b} reads {dl.blks[int(j)]}, which follows it in decode order"
    return True


def record_intra(name, p, blks, seed, patches=(), is_intra=None, pinned_by=None, rec=None):
    blks = list(blks)
    for b in blks:
        if b.tu is not None:
            b.tu.x, b.tu.y = b.x, b.y
    dl = D.record(name, p, [], [], seed, pinned_by=pinned_by, rec=rec, intra=blks, is_intra=is_intra, make=IntraList)
    dl.blks, dl.patches, dl.is_intra = blks, list(patches), is_intra
    assert dl.frame.n_intra == len(blks) and dl.frame.n_pu == 0
    check_contract(dl)
    return dl


def occupancy(dl):
    """[(CTU, sub-level, blocks <= 8x8, larger blocks)] read from the recorded frame's sub_start"""
    f, out = dl.frame, []
    for k in range(f.n_ictu):
        e = f.ictu[k]
        for s in range(e.n_sub):
            b0, b1 = f.sub_start[e.sub_first + s], f.sub_start[e.sub_first + s + 1]
            small = sum(f.intra[i].log2_size <= 3 for i in range(b0, b1))
            out.append((e.ctu, s, small, b1 - b0 - small))
    return out


# ---------------------------------------------------------------------------------------------------------- cell packing ----
def _cell(p, b, space):
    """side of the cell of a block: `space` x the side of the luma square it (with its lower half in 4:2:2) covers"""
    _, _, nh, nv = luma_rect(p, b.c, 0, 0, b.n)
    return space * max(nh, nv * (2 if b.lower is not None else 1))


def _place(p, b, CX, CY):
    hs, vs = F.hshift(p, b.c), F.vshift(p, b.c)
    b.cx, b.cy, b.x, b.y = CX, CY, CX >> hs, CY >> vs
    if b.lower is not None:
        b.lower.x, b.lower.y = b.x, b.y + b.n


def pack_cells(name, chroma, bd, blks, seed, space=2, dim=MAX_DIM, fill=0.9, pinned_by=None, finish=None, **pkw):
    """blocks (in the given, shuffled order) -> pictures of at most dim x dim, plane by plane: each block the top-left part of a cell
    of its own, the cells shelf-packed from (margin, margin) on, margin = the largest cell.  Inside a picture the list order is the
    shuffled one.  finish(p, blocks) may return (patches, is_intra) for the picture."""
    p_full = params(dim, dim, chroma, bd, **pkw)
    order = {id(b): i for i, b in enumerate(blks)}
    for b in blks:
        b.cell = _cell(p_full, b, space)
    margin = max(64, max(b.cell for b in blks))
    room = dim - margin
    queues = {c: [b for b in blks if b.c == c] for c in range(F.n_planes(p_full))}
    lists = []
    while any(queues.values()):
        here = []
        for c, q in queues.items():
            take, area = [], 0
            while q and area < fill * room * room:
                take.append(q.pop(0))
                area += take[-1].cell ** 2
            placed, rest = D.shelf_pack([(b.cell, b.cell) for b in take], room, room)
            assert placed or not take
            for i in sorted(placed):
                _place(p_full, take[i], margin + placed[i][0], margin + placed[i][1])
                here.append(take[i])
            queues[c] = sorted([take[i] for i in rest], key=lambda b: order[id(b)]) + q
        here.sort(key=lambda b: order[id(b)])
        height = (max(b.cy + b.cell for b in here) + 63) // 64 * 64
        p = params(dim, height, chroma, bd, **pkw)
        out = [x for b in here for x in ((b, b.lower) if b.lower is not None else (b,))]
        for b in out:                                         # a lower half keeps the flags of the upper one that it can have, and reads it
            if b.tag == "lower":
                b.avail &= zscan_avail(p, b.c, b.x, b.y, b.n)
        patches, is_intra = finish(p, out) if finish else ((), None)
        # constructed samples make the content the list's own: a seed of its own keeps it apart where pictures are shared by seed
        lists.append(record_intra(f"{name} picture {len(lists)}", p, out, seed + (100 * len(lists) if patches else 0), patches, is_intra, pinned_by=pinned_by))
    return lists


# ------------------------------------------------------------------------------------------------------------- family F ----
def f_matrix(chroma, full):
    """[(plane type: 0 luma, 1 chroma; log2 size; mode; flags)]"""
    out = []
    for pt, sizes in ((0, (2, 3, 4, 5)), (1, chroma_sizes(chroma))):
        for log2 in sizes:
            modes = range(35) if full or log2 < 5 else CUT_MODES_32
            out += [(pt, log2, m, a) for m in modes for a in range(32)]
    return out


@functools.lru_cache(maxsize=64)
def build_f(chroma, bd, part=None, pinned_by=None):
    """every (plane type, size, mode, flags) once, each block alone in its cell on extreme-mixed noise; residuals cycle through none /
    small random / DC coefficient +-32767 (F_KINDS), the cycle shifted by one from format to format.  Chroma blocks alternate between Cb and Cr; in 4:2:2 a chroma block is the upper half of the
    vertical pair of its transform unit and the lower half (same mode, the upper half's flags plus `up`, as far as it can have them)
    reads it.  Shuffled and dealt to F_PARTS parts (part=None: all of them)."""
    parts = F_PARTS[(chroma, bd)]
    if part is None:
        return [dl for k in range(parts) for dl in build_f(chroma, bd, k, pinned_by)]
    matrix = f_matrix(chroma, (chroma, bd) in F_FULL)
    shift = (F_FULL + F_CUT).index((chroma, bd))               # see F_KINDS
    rng = np.random.default_rng(7000 + 16 * chroma + bd)
    perm = rng.permutation(len(matrix))
    blks = []
    for i in perm[part::parts]:
        i = int(i)
        pt, log2, mode, avail = matrix[i]
        r = np.random.default_rng([7100 + 16 * chroma + bd, i])
        c = 0 if not pt else 1 + (i & 1)
        kind = F_KINDS[(i + shift) % len(F_KINDS)]
        b = Blk(c, log2, mode, avail, make_res(r, kind, log2, c, bd), note="[F]")
        b.tag = (pt, log2, mode, avail)
        if pt and chroma == 2:
            b.lower = Blk(c, log2, mode, avail | U, make_res(r, (1, 0, 3, 2)[i % 4], log2, c, bd), note="[F: lower half of a 4:2:2 pair]")
            b.lower.tag = "lower"
        blks.append(b)
    return pack_cells(f"F chroma {chroma} {bd} bit part {part}", chroma, bd, blks, seed=21, pinned_by=pinned_by)


def f_triples(lists):
    """[(plane type, log2 size, mode, flags)] of the blocks of the matrix (lower halves of 4:2:2 pairs left out), with repeats"""
    return [b.tag for dl in lists for b in dl.blks if isinstance(b.tag, tuple)]


# ------------------------------------------------------------------------------------------------------------- family G ----
def _g_planes(chroma):
    return [0] + ([1, 2] if chroma else [])


def _g_sizes(chroma, c):
    return (2, 3, 4, 5) if c == 0 else chroma_sizes(chroma)


def cut_values(p_chroma, c, n):
    """the lengths 0 < v < n, multiples of 4, at which a plane's edge can cut the run beside an n x n block: the picture's width and
    height are multiples of 8 luma samples, so in a plane that is not subsampled only multiples of 8 occur"""
    sub = 1 if c and p_chroma in (1, 2) else 0
    return [v for v in range(4, n, 4) if ((3 * n + v) << sub) % 8 == 0]


def cut_values_v(p_chroma, c, n):
    sub = 1 if c and p_chroma == 1 else 0
    return [v for v in range(4, n, 4) if ((3 * n + v) << sub) % 8 == 0]


@functools.lru_cache(maxsize=32)
def build_g(chroma, bd, what):
    """what = "tr": blocks in the last columns whose up-right run the picture's edge cuts to 0 < tr_size < N (every possible multiple of
    4), stacked in one column of cells; "bl": the transpose; "origin": blocks at (0, 0), at x = 0 and at y = 0 with every subset of
    the flags the position allows; "tiny": pictures of 8x8, 16x8 and 8x16 tiled with blocks that carry their true flags.
    Modes G_MODES, sizes 4 .. 32 (the slot path and a wave each); every block has no residual or a small one, drawn, so that
    the prediction shows in the picture."""
    rng = np.random.default_rng(8000 + 16 * chroma + bd + 100 * G_KINDS.index(what))
    hsv = lambda c: (int(bool(c) and chroma in (1, 2)), int(bool(c) and chroma == 1))
    lists, k = [], 0
    if what in ("tr", "bl"):
        hor = what == "tr"
        for c in _g_planes(chroma):
            hs, vs = hsv(c)
            for log2 in _g_sizes(chroma, c):
                n = 1 << log2
                combos = [(m, a) for m in G_MODES for a in ((ALL5, U | UR) if hor else (ALL5, L | BL))]
                per = max(1, min(len(combos), (MAX_DIM >> (vs if hor else hs)) // (2 * n) - 1))
                for v in (cut_values if hor else cut_values_v)(chroma, c, n):
                    for i0 in range(0, len(combos), per):
                        here = combos[i0:i0 + per]
                        along, across = 2 * n * (len(here) + 1), 3 * n + v
                        pw, ph = (across, along) if hor else (along, across)
                        p = params(pw << hs, ph << vs, chroma, bd)
                        blks = []
                        for j, (m, a) in enumerate(here, 1):
                            k += 1
                            x, y = (2 * n, 2 * n * j) if hor else (2 * n * j, 2 * n)
                            b = Blk(c, log2, m, a, make_res(rng, int(rng.integers(2)), log2, c, bd), f"[G: {what}_size {v}]", x, y)
                            b.edge = (what, log2, v)
                            blks.append(b)
                        lists.append(record_intra(f"G {what} chroma {chroma} {bd} bit plane {c} {n}x{n} cut {v} list {i0 // per}", p, blks, seed=22))
    elif what == "origin":
        for c in _g_planes(chroma):
            hs, vs = hsv(c)
            for log2 in _g_sizes(chroma, c):
                n = 1 << log2
                cells = max(2, min(5, (MAX_DIM >> max(hs, vs)) // (2 * n)))
                p = params((2 * n * cells) << hs, (2 * n * cells) << vs, chroma, bd)
                combos = [(m, s) for m in G_MODES for s in range(4)]
                for i0 in range(0, len(combos), cells - 1):
                    here = combos[i0:i0 + cells - 1]
                    blks = [Blk(c, log2, here[0][0], 0, make_res(rng, int(rng.integers(2)), log2, c, bd), "[G: at (0, 0)]", 0, 0)]
                    for j, (m, s) in enumerate(here, 1):
                        for x, y, bits in ((0, 2 * n * j, (U, UR)), (2 * n * j, 0, (L, BL))):
                            k += 1
                            real = zscan_avail(p, c, x, y, n)
                            assert real == bits[0] | bits[1], (c, x, y, n, real)
                            a = (bits[0] if s & 1 else 0) | (bits[1] if s & 2 else 0)
                            blks.append(Blk(c, log2, m, a, make_res(rng, int(rng.integers(2)), log2, c, bd), f"[G: at {'x' if x == 0 else 'y'} = 0]", x, y))
                    lists.append(record_intra(f"G origin chroma {chroma} {bd} bit plane {c} {n}x{n} list {i0 // (cells - 1)}", p, blks, seed=22))
    else:
        for w, h in ((8, 8), (16, 8), (8, 16)):
            p = params(w, h, chroma, bd)
            for li, m0 in enumerate(range(0, len(G_MODES), 3)):
                for small in (0, 1):
                    blks = []
                    for Y in range(0, h, 8):
                        for X in range(0, w, 8):
                            luma = [(X + dx, Y + dy, 2) for dy in (0, 4) for dx in (0, 4)] if small else [(X, Y, 3)]
                            units = [(0, x, y, l2) for x, y, l2 in luma]
                            if chroma == 3:
                                units = [(c, x, y, l2) for x, y, l2 in luma for c in (0, 1, 2)]
                            elif chroma == 2:
                                units += [(c, X // 2, Y + dy, 2) for c in (1, 2) for dy in (0, 4)]
                            elif chroma == 1:
                                units += [(c, X // 2, Y // 2, 2) for c in (1, 2)]
                            for c, x, y, l2 in units:
                                k += 1
                                m = G_MODES[(m0 + k) % len(G_MODES)]
                                blks.append(Blk(c, l2, m, zscan_avail(p, c, x, y, 1 << l2), make_res(rng, int(rng.integers(2)), l2, c, bd), "[G: tiny picture]", x, y))
                    lists.append(record_intra(f"G tiny {w}x{h} chroma {chroma} {bd} bit list {li} {'4x4' if small else '8x8'}", p, blks, seed=22))
    return lists


def g_cuts(lists):
    """{(what, log2 size, plane type): {cut length}}"""
    out = {}
    for dl in lists:
        for b in dl.blks:
            if b.edge:
                out.setdefault((b.edge[0], b.edge[1], int(b.c > 0)), set()).add(b.edge[2])
    return out


# ------------------------------------------------------------------------------------------------------------- family H ----
H_VARIANTS = {"strong": {}, "plain": {"strong_intra_smoothing": 0}, "disabled": {"intra_smoothing_disabled": 1}}


@functools.lru_cache(maxsize=64)
def build_h_thr(bd, variant="strong", chroma=1, plane=0):
    """N x N blocks (32x32 in luma and in a 4:4:4 chroma plane, 16x16 in a 4:2:0 chroma plane), nine to a picture: t = |top[-1] +
    top[2N-1] - 2 top[N-1]| and l (the same of the left column) take lim - 1, lim, lim + 1 in all nine pairs, lim = 1 << (bd - 5); one
    picture per sign pair of the inner expressions and per flag set of H_FLAGS (with up-right / bottom-left cleared the end of the edge
    is the substituted middle and the expression becomes corner - middle).  The same blocks and content for every variant; no residual
    or a small one, so that the smoothing decision shows in the picture."""
    lim, mx = 1 << (bd - 5), (1 << bd) - 1
    log2 = 5 if plane == 0 or chroma == 3 else 4
    n = 1 << log2
    sub = 1 if plane and chroma == 1 else 0
    side = (4 * n * 3 + 2 * n) << sub                          # cells of 4N, so that the constructed edges of two blocks do not meet
    p = params(side, side, chroma, bd, **H_VARIANTS[variant])
    lists = []
    for si, (st, sl) in enumerate(H_SIGNS):
        for fi, avail in enumerate(H_FLAGS):
            rng = np.random.default_rng([9000 + bd, si, fi, chroma, plane])
            blks, patches = [], []
            for k in range(9):
                vt, vl = lim - 1 + k % 3, lim - 1 + k // 3
                x, y = 2 * n + 4 * n * (k % 3), 2 * n + 4 * n * (k // 3)
                while True:                                   # the two edges share the corner
                    c0, a, a2, e, e2 = (int(t) for t in rng.integers(0, mx + 1, 5))
                    if avail & UR:
                        e = st * vt + 2 * a - c0
                    else:
                        a = c0 - st * vt
                    if avail & BL:
                        e2 = sl * vl + 2 * a2 - c0
                    else:
                        a2 = c0 - sl * vl
                    if all(0 <= t <= mx for t in (a, a2, e, e2)):
                        break
                top = rng.integers(0, mx + 1, 2 * n + 1)
                left = rng.integers(0, mx + 1, 2 * n)
                top[0], top[n], top[2 * n] = c0, a, e
                left[n - 1], left[2 * n - 1] = a2, e2
                dt = np.uint8 if bd == 8 else np.uint16
                patches += [(plane, x - 1, y - 1, top.astype(dt)[None, :]), (plane, x - 1, y, left.astype(dt)[:, None])]
                b = Blk(plane, log2, H_MODES[(k + si + 2 * fi) % len(H_MODES)], avail, make_res(rng, (k + k // 3 + si) % 2, log2, plane, bd),
                        f"[H: t = lim{vt - lim:+d}, l = lim{vl - lim:+d}, signs {st:+d} {sl:+d}, {variant}]", x, y)
                b.edge = (vt, vl)
                blks.append(b)
            lists.append(record_intra(f"H thresholds {bd} bit chroma {chroma} plane {plane} {variant} signs {si} flags {avail:05b}", p, blks,
                                      seed=2300 + 16 * si + fi, patches=patches))
    return lists


def h_measure(dl, b):
    """(t, l, sign of t's inner expression, of l's) of a block of build_h_thr, computed from the list's picture and the block's flags"""
    pl = dl.pictures()[2].planes[b.c].astype(np.int64)
    n, x, y = b.n, b.x, b.y
    corner, tm, lm = pl[y - 1, x - 1], pl[y - 1, x + n - 1], pl[y + n - 1, x - 1]
    te = pl[y - 1, x + 2 * n - 1] if b.avail & UR else tm
    le = pl[y + 2 * n - 1, x - 1] if b.avail & BL else lm
    ti, li = corner + te - 2 * tm, corner + le - 2 * lm
    return abs(int(ti)), abs(int(li)), int(np.sign(ti)), int(np.sign(li))


@functools.lru_cache(maxsize=8)
def build_h_clip(bd):
    """modes 1, 10 and 26 at 4x4 .. 16x16 in luma with top[], left[] and the corner each at 0 or the maximum, all eight arrangements:
    top[0] + ((left[y] - left[-1]) >> 1) and its transpose go below 0 and above the maximum"""
    mx = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    rng = np.random.default_rng(9500 + bd)
    blks = []
    for log2 in (2, 3, 4):
        for mode in (1, 10, 26):
            for arr in range(8):
                b = Blk(0, log2, mode, ALL5, make_res(rng, (0, 0, 1)[arr % 3], log2, 0, bd),
                        f"[H: top {mx * (arr & 1)}, left {mx * (arr >> 1 & 1)}, corner {mx * (arr >> 2 & 1)}]")
                b.edge = arr
                blks.append(b)
    blks = [blks[i] for i in rng.permutation(len(blks))]

    def finish(p, out):
        patches = []
        for b in out:
            n, arr = b.n, b.edge
            top = np.full(2 * n + 1, mx * (arr & 1), dt)
            top[0] = mx * (arr >> 2 & 1)
            patches += [(0, b.x - 1, b.y - 1, top[None, :]), (0, b.x - 1, b.y, np.full((2 * n, 1), mx * (arr >> 1 & 1), dt))]
        return patches, None
    return pack_cells(f"H clip {bd} bit", 1, bd, blks, seed=24, space=4, finish=finish)


# ------------------------------------------------------------------------------------------------------------- family J ----
def _j_unit(rng, p, X, Y, size, split_pct, out):
    chroma = p.chroma_format_idc

    def blk(c, x, y, log2):
        r = int(rng.integers(100))
        kind = 4 if r < 22 else 5 if r < 44 else 1 if r < 60 else 0
        mode = J_MODES[int(rng.integers(len(J_MODES)))]
        out.append(Blk(c, log2, mode, zscan_avail(p, c, x, y, 1 << log2), make_res(rng, kind, log2, c, p.bit_depth), "[J]", x, y))
    if size > 32 or (size > 8 and rng.integers(100) < split_pct):
        for dy in (0, size // 2):
            for dx in (0, size // 2):
                _j_unit(rng, p, X + dx, Y + dy, size // 2, split_pct, out)
        return
    log2 = size.bit_length() - 1
    if size == 8 and rng.integers(100) < split_pct:            # four 4x4 luma blocks
        for dy in (0, 4):
            for dx in (0, 4):
                blk(0, X + dx, Y + dy, 2)
                if chroma == 3:
                    blk(1, X + dx, Y + dy, 2)
                    blk(2, X + dx, Y + dy, 2)
        if chroma == 1:
            blk(1, X // 2, Y // 2, 2)
            blk(2, X // 2, Y // 2, 2)
        return
    blk(0, X, Y, log2)
    for c in (1, 2):
        blk(c, X >> (chroma == 1), Y >> (chroma == 1), log2 - (chroma == 1))


@functools.lru_cache(maxsize=8)
def build_j(chroma, bd):
    """CTUs of 16, 32 and 64 covered by a random quadtree of blocks in decode order with their true z-scan flags: one CTU, one row of
    four, 3 x 3; modes J_MODES; 44 % of the blocks are driven to 0 or to the maximum by their residual, so that the next block gathers
    saturated neighbours.  The split probability changes from CTU to CTU, which varies how many small blocks a sub-level holds."""
    lists = []
    for lc in (4, 5, 6):
        ctb = 1 << lc
        for cw, ch in ((1, 1), (4, 1), (3, 3)):
            for seed in (0, 1):
                rng = np.random.default_rng([10000 + 16 * chroma + bd, lc, cw, ch, seed])
                p = F.pic_params(cw * ctb, ch * ctb, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc, sao=0, deblock=0, transquant_bypass_enable=1)
                blks = []
                for cy in range(ch):
                    for cx in range(cw):
                        _j_unit(rng, p, cx * ctb, cy * ctb, ctb, (15, 35, 55, 75, 90)[int(rng.integers(5))], blks)
                lists.append(record_intra(f"J chroma {chroma} {bd} bit CTU {ctb} {cw}x{ch} seed {seed}", p, blks, seed=25 + seed))
    return lists


# ------------------------------------------------------------------------------------------------------------- family K ----
def k_groups(p, b):
    """the groups of four samples of the edges of block b as luma rectangles (X, Y, w, h), in mask-bit order: the left column from the
    top to the end of bottom-left, the corner, the top row to the end of up-right; groups outside the picture are None"""
    hs, vs = F.hshift(p, b.c), F.vshift(p, b.c)
    n, out = b.n, []
    rects = [(b.x - 1, b.y + 4 * g, 1, 4) for g in range(n // 2)] + [(b.x - 1, b.y - 1, 1, 1)] + [(b.x + 4 * g, b.y - 1, 4, 1) for g in range(n // 2)]
    for x, y, w, h in rects:
        X, Y = x << hs, y << vs
        out.append((X, Y, w << hs, h << vs) if 0 <= X < p.width and 0 <= Y < p.height else None)
    return out


def k_map(p, blks):
    """the min-PU map of a picture: every block's own cells intra, bit i of its mask = group i of its edges intra"""
    lpu = p.log2_min_pu_size
    m = np.zeros((p.height >> lpu, p.width >> lpu), np.uint8)

    def put(X, Y, w, h, v):
        m[Y >> lpu:((Y + h - 1) >> lpu) + 1, X >> lpu:((X + w - 1) >> lpu) + 1] = v
    for b in blks:
        for i, g in enumerate(k_groups(p, b)):
            if g is not None:
                put(*g, (b.mask >> i) & 1)
    for b in blks:
        put(*luma_rect(p, b.c, b.x, b.y, b.n), 1)
    return m


def _k_finish(p, out):
    return (), k_map(p, out)


@functools.lru_cache(maxsize=8)
def build_k8(bd=8, log2_min_cb=3, part=None, pinned_by=None):
    """8x8 luma blocks, all five flags realisable, under every one of the 512 masks over (four left groups down to the end of
    bottom-left, the corner, four top groups): all flags for every mask, three other flag sets on a rotating quarter of the masks;
    modes cycle through K_MODES; no residual or a small one, drawn (as in all of K: a saturating one would hide the prediction).  With log2_min_cb = 4 (8x8 min PUs: two groups share a map cell) every fourth mask.  Four parts."""
    if part is None:
        return [dl for k in range(4) for dl in build_k8(bd, log2_min_cb, k, pinned_by)]
    rng = np.random.default_rng(11000 + bd + log2_min_cb)
    combos = [(mask, ALL5) for mask in range(512)] + [(mask, K_SUBSETS[s]) for s in range(3) for mask in range(512) if mask % 4 == (s + mask // 4) % 4]
    if log2_min_cb == 4:
        combos = combos[::4]
    blks = []
    for i in rng.permutation(len(combos))[part::4]:
        mask, avail = combos[int(i)]
        b = Blk(0, 3, K_MODES[int(i) % len(K_MODES)], avail, make_res(rng, int(rng.integers(2)), 3, 0, bd), f"[K: mask {mask:09b}]")
        b.mask = mask
        blks.append(b)
    return pack_cells(f"K 8x8 {bd} bit min cb {1 << log2_min_cb} part {part}", 1, bd, blks, seed=26, space=4, finish=_k_finish, pinned_by=pinned_by,
                      constrained_intra_pred=1, log2_min_cb_size=log2_min_cb)


def k_big_masks(rng, groups):
    full = (1 << groups) - 1
    alt = sum(1 << i for i in range(0, groups, 2))
    return ([full, 0, alt, full ^ alt] + [1 << i for i in range(groups)] + [full ^ (1 << i) for i in range(groups)] +
            [int(v) for v in rng.integers(0, full + 1, 64, dtype=np.int64)])


@functools.lru_cache(maxsize=8)
def build_k_big(chroma, bd, part=None):
    """16x16 and 32x32 luma blocks and 4x4 / 8x8 / 16x16 chroma blocks under the masks all, none, alternating (both phases), a single
    intra group at each position, a single inter group at each position and 64 drawn ones; all five flags; three parts"""
    if part is None:
        return [dl for k in range(3) for dl in build_k_big(chroma, bd, k)]
    rng = np.random.default_rng(12000 + 16 * chroma + bd)
    blks = []
    for c, log2 in [(0, 4), (0, 5)] + [(1 + (l2 & 1), l2) for l2 in (2, 3, 4)]:
        for j, mask in enumerate(k_big_masks(rng, (1 << log2) + 1)):
            b = Blk(c, log2, K_MODES[j % len(K_MODES)], ALL5, make_res(rng, int(rng.integers(2)), log2, c, bd), f"[K: mask {mask:b}]")
            b.mask = mask
            blks.append(b)
    blks = [blks[i] for i in rng.permutation(len(blks))[part::3]]
    return pack_cells(f"K large chroma {chroma} {bd} bit part {part}", chroma, bd, blks, seed=27, space=4, dim=384, finish=_k_finish, constrained_intra_pred=1)


@functools.lru_cache(maxsize=8)
def build_k_edge(chroma, bd):
    """blocks at x = 0 (the reference zero-fills the left column, hevcpred_template.c:236), at y = 0 and at (0, 0) under drawn masks,
    with the flags the position allows and with subsets of them"""
    rng = np.random.default_rng(13000 + 16 * chroma + bd)
    lists = []
    for c, log2 in [(0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (2, 3), (1, 4)]:
        n = 1 << log2
        hs, vs = int(chroma == 1 and c > 0), int(chroma == 1 and c > 0)
        p = params((4 * n * 4) << hs, (4 * n * 4) << vs, chroma, bd, constrained_intra_pred=1)
        for li in range(6):
            blks = []
            for j in range(4):
                for x, y in ((0, 4 * n * j), (4 * n * j, 0)) if j else ((0, 0),):
                    real = zscan_avail(p, c, x, y, n)
                    a = real if (li + j) % 3 else real & int(rng.integers(32))
                    b = Blk(c, log2, K_MODES[(li + j) % len(K_MODES)], a, make_res(rng, int(rng.integers(2)), log2, c, bd), "[K: picture edge]", x, y)
                    b.mask = int(rng.integers(0, 1 << (n + 1), dtype=np.int64)) if li else (1 << (n + 1)) - 1
                    blks.append(b)
            lists.append(record_intra(f"K edge chroma {chroma} {bd} bit plane {c} {n}x{n} list {li}", p, blks, seed=28, is_intra=k_map(p, blks)))
    return lists
