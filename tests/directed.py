"""Directed extreme-value work lists for the inter and the residual pass (builders only: no GPU, no reference).

The random generator (openhevc_amd/synth/synth.c) never draws the values at which mc_kernel and residual_kernel can go wrong:
full-range weights and offsets, dense or sign-aligned saturating coefficient blocks, every fraction x job shape x kind, windows
that cross a plane's edge by a chosen number of samples, job counts that leave quarters of a wave dead.  The families below
enumerate them.  Every list is recorded through the recorder's C ABI with the in-loop filters off, so the picture IS the output
of the passes; tests/test_directed_lists.py holds the lists against their own coverage claims (and, where the reference is
present, the checker against the reference's slots on them), tests/test_gpu_directed.py holds the engine against the checker.

  A  fraction x shape x kind matrix       build_a(chroma, bd, full)
  B  borders and clamping                 build_b(chroma, bd)
  C  weights                              build_c(chroma, bd)
  D  wave occupancy                       build_d(chroma, bd)
  E  residual extremes                    build_e(chroma, bd)

and two models: idct_model (m1), expected_pu (m2).
"""
import ctypes as C
import functools

import numpy as np

from openhevc_amd import frame as F
from oracle_lib import i16p, off_u8p, pix_dtype, rand_pixels, u8p

# ---------------------------------------------------------------------------------------------------------------- tables ----
SHAPES_ALL = [(8, 4), (4, 8), (8, 8), (16, 8), (8, 16), (16, 16), (16, 4), (16, 12), (4, 16), (12, 16), (32, 16), (16, 32), (32, 32),
              (32, 8), (32, 24), (8, 32), (24, 32), (64, 32), (32, 64), (64, 64), (64, 16), (64, 48), (16, 64), (48, 64)]
SHAPES_CUT = [(8, 4), (4, 8), (8, 8), (12, 16), (16, 12), (16, 16), (32, 8), (24, 32)]
KINDS = ("uni0", "uni1", "bi", "wuni", "wbi")
A_FULL = [(1, 8), (1, 10)]                                    # (chroma_format_idc, bit depth): all 24 shapes
A_CUT = [(1, 12), (2, 10), (3, 8), (3, 12), (0, 8)]           # the cut shape set

# (log2 denominator luma, chroma, w0, o0, w1, o1), the same for the three components
GRADED = [(7, 7, 255, -128, -128, 127), (7, 7, -128, 127, 255, -128), (0, 0, 1, 127, 1, -128), (0, 7, 2, -128, -1, 127),
          (7, 0, 127, -128, 129, 127), (0, 0, -1, 127, 2, -128), (6, 7, 64, 0, 64, 0), (7, 6, 128, 1, 128, -1), (1, 0, 3, -128, -1, 127)]
SATURATING = [(3, 4, -128, 127, 127, 127), (7, 7, 0, 127, 0, -128), (5, 5, 255, -128, -128, -128)]

B_SIZES = [(8, 8), (16, 8), (8, 16), (24, 16), (64, 64)]
B_FORMATS = [(1, 8), (2, 10), (3, 12)]
B_FRACS = [(0, 0), (1, 0), (0, 3), (2, 2), (5, 7)]
ZONES = {"inside": (0, 0), "left": (-1, 0), "right": (1, 0), "top": (0, -1), "bottom": (0, 1),
         "top_left": (-1, -1), "top_right": (1, -1), "bottom_left": (-1, 1), "bottom_right": (1, 1)}
CROSSINGS = (1, 2, 3, 4, 7, 8, "outside")
INT16_EXTREMES = [(-32768, None), (32767, None), (None, -32768), (None, 32767),
                  (-32768, -32768), (-32768, 32767), (32767, -32768), (32767, 32767)]
B_VARIANTS = [("inside", 0)] + [(z, c) for z in list(ZONES)[1:] for c in CROSSINGS] + [("int16", e) for e in INT16_EXTREMES]

C_FORMATS = [(cf, bd) for cf in (1, 3) for bd in (8, 10, 12)]
C_KINDS = ("uni0", "uni1", "bi")
C_SHAPES = [(8, 8), (12, 16)]
C_REPLICAS = 4                                                # PUs per (entry, kind, shape): 4 x (64 + 192) luma samples per cell
D_FORMATS = [(1, 8), (3, 10)]
E_FORMATS = [(1, 8), (1, 10), (1, 12), (3, 10)]
E_EDGES = (0, 3, 4, 7, 8, 15, 16, 31)                         # the edges of the bounding box residual_kernel derives for >= 16x16
E_DENSE = 8                                                   # e1 blocks per (bit depth, size) cell
SECOND_CLIP_CELLS = {(10, 32), (12, 8), (12, 16), (12, 32)}   # (bit depth, size) where an e2 block reaches the second clip

_DCT_C = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4]
_DST7 = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)


# -------------------------------------------------------------------------------------------------------------- records ----
class Pu:
    """one recorded prediction unit and what it was chosen for"""
    __slots__ = ("x", "y", "w", "h", "kind", "mv", "wt", "note")

    def __init__(self, w, h, kind, mv, wt=None, note="", x=0, y=0):
        self.x, self.y, self.w, self.h, self.kind, self.mv, self.wt, self.note = x, y, w, h, kind, mv, wt, note

    @property
    def refs(self):
        """(index into ref_pics for list 0, for list 1), -1 = list not used"""
        return {"uni0": (0, -1), "uni1": (-1, 1), "bi": (0, 1)}[self.kind]

    def frac(self, l=0):
        return self.mv[l][0] & 7, self.mv[l][1] & 7

    def __repr__(self):
        f = " / ".join(f"mv {self.mv[l]} fraction {self.frac(l)}" for l in (0, 1) if self.refs[l] >= 0)
        return f"PU {self.w}x{self.h} at ({self.x}, {self.y}) {self.kind} {f} weights {self.wt} {self.note}"


class Tu:
    """one recorded residual block: `intra` blocks are the residual of a DC-mode intra block, the others are added at once"""
    __slots__ = ("c", "x", "y", "log2", "kind", "flags", "coeffs", "intra", "recipe")

    def __init__(self, log2, kind, flags, coeffs, recipe, c=0, intra=False):
        self.c, self.x, self.y, self.log2, self.kind, self.flags, self.intra, self.recipe = c, 0, 0, log2, kind, flags, intra, recipe
        self.coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)

    def __repr__(self):
        n = 1 << self.log2
        kind = ("IDCT", "DST4", "skip", "bypass", "PCM")[self.kind]
        return (f"TU {n}x{n} plane {self.c} at ({self.x}, {self.y}) {kind} flags {self.flags} "
                f"{'intra DC residual' if self.intra else 'inter (added at once)'}: {self.recipe}")


class DirectedList:
    """a recorded work list (kept alive by a FrameCopy) with the description of every item in it"""

    def __init__(self, name, p, fc, pus, tus, seed):
        self.name, self.p, self.fc, self.pus, self.tus, self.seed = name, p, fc, pus, tus, seed

    @property
    def frame(self):
        return self.fc.frame

    def pictures(self):
        """{0, 1: reference pictures, 2: the current picture's initial content}: extreme-mixed noise, the same for the lists of
        one geometry, format and seed"""
        base = _base_pictures(self.p.width, self.p.height, self.p.chroma_format_idc, self.p.bit_depth, self.seed)
        return {k: hp.copy() for k, hp in enumerate(base)}

    def item_at(self, c, x, y):
        """the description of the item that wrote sample (x, y) of plane c"""
        hs, vs = F.hshift(self.p, c), F.vshift(self.p, c)
        hit = [repr(t) for t in self.tus if t.c == c and t.x <= x < t.x + (1 << t.log2) and t.y <= y < t.y + (1 << t.log2)]
        hit += [repr(u) for u in self.pus if u.x >> hs <= x < (u.x + u.w) >> hs and u.y >> vs <= y < (u.y + u.h) >> vs]
        return "; ".join(hit) if hit else "no item (initial content)"


MAX_DIM = 256                                                 # pictures of A and E are at most this wide and high


@functools.lru_cache(maxsize=16)
def _base_pictures(width, height, chroma, bd, seed):
    p = F.pic_params(width, height, bit_depth=bd, chroma_format_idc=chroma, sao=0, deblock=0)
    rng = np.random.default_rng(seed)
    pics = []
    for _ in range(3):
        hp = F.HostPic(p)
        hp.planes = [rand_pixels(rng, pl.shape, bd, extreme=True) for pl in hp.planes]
        pics.append(hp)
    return tuple(pics)


def make_weights(entry):
    dl, dc, w0, o0, w1, o1 = entry
    wp = F.OhWeights()
    for c in range(3):
        wp.w[0][c], wp.w[1][c], wp.o[0][c], wp.o[1][c] = w0, w1, o0, o1
    wp.log2_denom[0], wp.log2_denom[1] = dl, dc
    return wp


def params(width, height, chroma, bd):
    return F.pic_params(width, height, bit_depth=bd, chroma_format_idc=chroma, sao=0, deblock=0, transquant_bypass_enable=1)


def record(name, p, pus, tus, seed, pinned_by=None, rec=None, intra=(), is_intra=None, make=None):
    """the items through oh_rec_begin / oh_rec_pu / oh_rec_tu / oh_rec_intra / oh_rec_finish, in the order given.  `intra`: blocks
    with c, x, y, log2, mode, avail and tu (a Tu or None), recorded after `tus` (tests/directed_intra.py); `is_intra`: the min-PU map
    of a picture with constrained intra prediction; `make`: the class of the result (DirectedList)"""
    lib = F.host()
    own = rec is None
    if own:
        rec = F.Recorder(p)
    refs = (C.c_int32 * F.OH_MAX_REFS)(*([0, 1] + [-1] * (F.OH_MAX_REFS - 2)))
    lib.oh_rec_begin(rec.h, 2, refs, F.OH_MAX_REFS)
    for u in pus:
        r0, r1 = u.refs
        wp = C.byref(make_weights(u.wt)) if u.wt is not None else None
        rc = lib.oh_rec_pu(rec.h, u.x, u.y, u.w, u.h, r0, u.mv[0][0], u.mv[0][1], r1, u.mv[1][0], u.mv[1][1], wp)
        assert rc == 0, u
    for t in tus:
        idx = lib.oh_rec_tu(rec.h, t.c, t.x, t.y, t.log2, t.kind, t.flags | (0 if t.intra else F.TUF_ADD_NOW), i16p(t.coeffs))
        assert idx != F.OH_NO_COEFF, t
        if t.intra:
            assert lib.oh_rec_intra(rec.h, t.c, t.x, t.y, t.log2, 1, 0, idx) == 0, t           # DC mode, no neighbour available
    if is_intra is not None:
        m = np.ascontiguousarray(is_intra, dtype=np.uint8)
        assert m.shape == (p.height >> p.log2_min_pu_size, p.width >> p.log2_min_pu_size), name
        C.memmove(lib.oh_rec_is_intra(rec.h), m.ctypes.data, m.size)
    for b in intra:
        idx = F.OH_NO_COEFF
        if b.tu is not None:
            idx = lib.oh_rec_tu(rec.h, b.c, b.x, b.y, b.log2, b.tu.kind, b.tu.flags, i16p(b.tu.coeffs))
            assert idx != F.OH_NO_COEFF, b
        assert lib.oh_rec_intra(rec.h, b.c, b.x, b.y, b.log2, b.mode, b.avail, idx) == 0, b
    f = lib.oh_rec_finish(rec.h)
    assert f, name
    fc = F.FrameCopy(f.contents, pinned_by=pinned_by)
    if own:
        rec.close()
    return (make or DirectedList)(name, p, fc, list(pus), list(tus), seed)


def shelf_pack(sizes, width, height):
    """sizes: [(w, h)]; shelves of decreasing height from the top; returns ({index: (x, y)}, [indices that did not fit])"""
    order = sorted(range(len(sizes)), key=lambda i: (-sizes[i][1], -sizes[i][0]))
    x = y = shelf = 0
    placed, rest = {}, []
    for i in order:
        w, h = sizes[i]
        if x + w > width:
            x, y, shelf = 0, y + shelf, 0
        if y + h > height:
            rest.append(i)
            continue
        placed[i] = (x, y)
        x, shelf = x + w, max(shelf, h)
    return placed, rest


def _pack_pus(name, chroma, bd, pus, seed, width, pinned_by=None, fill=0.92):
    """PUs (in the given, shuffled order) -> as many pictures of at most width x MAX_DIM as needed; inside a picture the list order is
    the shuffled one, so a wave of mc_kernel mixes shapes, kinds and fractions"""
    lists, queue = [], list(pus)
    while queue:
        take, area = [], 0
        while queue and area < fill * width * MAX_DIM:
            take.append(queue.pop(0))
            area += take[-1].w * take[-1].h
        placed, rest = shelf_pack([(u.w, u.h) for u in take], width, MAX_DIM)
        assert placed
        queue = [take[i] for i in sorted(rest)] + queue
        here = [take[i] for i in sorted(placed)]
        for i in sorted(placed):
            take[i].x, take[i].y = placed[i]
        height = (max(u.y + u.h for u in here) + 63) // 64 * 64    # few distinct geometries: the pictures are shared
        lists.append(record(f"{name} picture {len(lists)}", params(width, height, chroma, bd), here, [], seed, pinned_by=pinned_by))
    return lists


# ------------------------------------------------------------------------------------------------------------- family A ----
A_PARTS = {True: 32, False: 10}                                # the matrix of a format is dealt to this many test cases (full / cut shape set)


@functools.lru_cache(maxsize=64)
def build_a(chroma, bd, full, part=None, pinned_by=None):
    """every (shape, kind, fraction) triple: fraction = (mvx & 7, mvy & 7) of the list in use — every luma quarter-sample pair
    and every chroma eighth-sample pair of the three chroma formats; the second list of a bi PU takes another fraction; weighted
    PUs cycle through the graded weight table, weighted uni PUs alternate between the lists.  Integer parts (mv >> 2) lie in
    -8 .. 7.  The PUs are shuffled and dealt to A_PARTS parts, each packed into pictures of its own (part=None: all parts)."""
    parts = A_PARTS[bool(full)]
    if part is None:
        return [dl for k in range(parts) for dl in build_a(chroma, bd, full, k, pinned_by)]
    shapes = SHAPES_ALL if full else SHAPES_CUT
    rng = np.random.default_rng(1000 + 16 * chroma + bd)
    n = len(shapes) * len(KINDS) * 64
    ks = rng.integers(-4, 4, size=(n, 4))
    pus = []
    for i in rng.permutation(n)[part::parts]:
        i = int(i)
        (w, h), kind, fr = shapes[i // 320], KINDS[(i // 64) % 5], i % 64
        fx, fy = fr & 7, fr >> 3
        kx0, ky0, kx1, ky1 = (int(v) for v in ks[i])
        mv0, mv1 = (fx + 8 * kx0, fy + 8 * ky0), (((fx + 3) & 7) + 8 * kx1, ((fy + 5) & 7) + 8 * ky1)
        base = {"wuni": ("uni0", "uni1")[(fr ^ (fr >> 3)) & 1], "wbi": "bi"}.get(kind, kind)
        if base == "uni1":
            mv0, mv1 = mv1, mv0                               # the list in use carries (fx, fy)
        wt = GRADED[(fr + i // 64) % len(GRADED)] if kind[0] == "w" else None
        pus.append(Pu(w, h, base, (mv0, mv1), wt, note=f"[A: {kind}]"))
    return _pack_pus(f"A chroma {chroma} {bd} bit part {part}", chroma, bd, pus, seed=11, width=MAX_DIM, pinned_by=pinned_by)


def a_triples(lists):
    """{(w, h, kind as asked for, fx, fy)} over the lists of one format"""
    out = set()
    for dl in lists:
        for u in dl.pus:
            l = 1 if u.kind == "uni1" else 0
            out.add((u.w, u.h, u.note[4:-1]) + u.frac(l))
            if u.kind == "bi":
                out.add((u.w, u.h, "list1 of " + u.note[4:-1]) + u.frac(1))
    return out


# ------------------------------------------------------------------------------------------------------------- family B ----
def _b_axis(side, crossing, pos, size, dim):
    """integer displacement that puts the 8-tap window of a block (samples pos-3 .. pos+size+3 before displacement) across the
    low (-1) / high (+1) edge of a plane `dim` wide by `crossing` samples, wholly outside by 64, or (0) as far inside as it goes"""
    if side == 0:
        lo, hi = 3 - pos, dim - 1 - (pos + size + 3)          # displacements that keep the window inside
        return (lo + hi) // 2 if lo <= hi else 0
    if crossing == "outside":
        return -(pos + size + 4) - 64 if side < 0 else dim + 3 - pos + 64
    return 3 - crossing - pos if side < 0 else dim + crossing - pos - size - 4


def b_mv(variant, x, y, w, h, width, height, frac):
    """the motion vector of one variant; the crossing holds for the luma window, the luma quarter-sample is frac & 3 and the
    eighth-sample bit (chroma of 4:2:0) follows the parity of the integer part"""
    zone, arg = variant
    if zone == "int16":
        small = (4 * _b_axis(0, 0, x, w, width) + (frac[0] & 3), 4 * _b_axis(0, 0, y, h, height) + (frac[1] & 3))
        return tuple(small[k] if arg[k] is None else arg[k] for k in (0, 1))
    sx, sy = ZONES[zone]
    return (4 * _b_axis(sx, arg, x, w, width) + (frac[0] & 3), 4 * _b_axis(sy, arg, y, h, height) + (frac[1] & 3))


def b_plan(width, height):
    """[(tiling offset, number of lists, step)]: 8x8 PUs on the 4-sample grid as tilings of non-overlapping positions.  List k of a
    tiling gives position j variant (step * k + j) % 65.  Pictures up to 24x16 and the aligned tiling of 64x64 run all 65 lists
    (every position meets every variant); the three offset tilings of 64x64 run 13 lists (every variant at some position of each)."""
    plan = []
    for oy in (0, 4):
        for ox in (0, 4):
            if ox + 8 > width or oy + 8 > height:
                continue
            whole = (width, height) != (64, 64) or (ox, oy) == (0, 0)
            plan.append(((ox, oy), len(B_VARIANTS) if whole else 13, 1 if whole else 5))
    return plan


B_PARTS = {(8, 8): 1, (16, 8): 2, (8, 16): 2, (24, 16): 4, (64, 64): 13}      # the lists of a picture size are dealt to this many test cases


@functools.lru_cache(maxsize=128)
def build_b(chroma, bd, size=None, part=None):
    """the lists of one format (size=None), of one picture size (part=None) or one part of those"""
    if size is None:
        return [dl for sz in B_SIZES for dl in build_b(chroma, bd, sz)]
    if part is None:
        return [dl for k in range(B_PARTS[size]) for dl in build_b(chroma, bd, size, k)]
    width, height = size
    p = params(width, height, chroma, bd)
    rec = F.Recorder(p)
    lists, nv, n = [], len(B_VARIANTS), 0
    for (ox, oy), n_lists, step in b_plan(width, height):
        positions = [(x, y) for y in range(oy, height - 7, 8) for x in range(ox, width - 7, 8)]
        for k in range(n_lists):
            n += 1
            if (n - 1) % B_PARTS[size] != part:
                continue
            rng = np.random.default_rng([2000 + 16 * chroma + bd, width, height, ox, oy, k])
            draw = rng.integers(0, [nv, 5, 5, 4], size=(len(positions), 4))
            pus = []
            for j, (x, y) in enumerate(positions):
                v0, v1 = B_VARIANTS[(step * k + j) % nv], B_VARIANTS[int(draw[j, 0])]
                f0, f1 = B_FRACS[int(draw[j, 1])], B_FRACS[int(draw[j, 2])]
                kind = ("uni0", "uni1", "bi", "bi")[int(draw[j, 3])]
                mv0, mv1 = b_mv(v0, x, y, 8, 8, width, height, f0), b_mv(v1, x, y, 8, 8, width, height, f1)
                note = f"[B: {v0[0]} {v0[1]}]" + (f" second list [{v1[0]} {v1[1]}]" if kind == "bi" else "")
                if kind == "uni1":
                    mv0, mv1 = mv1, mv0
                pus.append(Pu(8, 8, kind, (mv0, mv1), None, note, x, y))
            lists.append(record(f"B {width}x{height} chroma {chroma} {bd} bit tiling ({ox}, {oy}) list {k}", p, pus, [], seed=12, rec=rec))
    rec.close()
    return lists


def b_pairs(lists):
    """{(width, height): {(zone, crossing)}} of the first variant of every PU"""
    out = {}
    for dl in lists:
        s = out.setdefault((dl.p.width, dl.p.height), set())
        for u in dl.pus:
            zone, arg = u.note[4:u.note.index("]")].split(" ", 1)
            s.add((zone, arg))
    return out


def _small_mv(rng, fx, fy):
    """fraction (mv & 7) as given, luma integer part (mv >> 2) in -8 .. 7"""
    kx, ky = (int(v) for v in rng.integers(-4, 4, 2))
    return (fx + 8 * kx, fy + 8 * ky)


# ------------------------------------------------------------------------------------------------------------- family C ----
@functools.lru_cache(maxsize=8)
def build_c(chroma, bd):
    """the weight table x uni L0 / uni L1 / bi x 8x8 / 12x16, C_REPLICAS PUs each with their own fractional vectors: one picture"""
    rng = np.random.default_rng(3000 + 16 * chroma + bd)
    pus = []
    for e, entry in enumerate(GRADED + SATURATING):
        for kind in C_KINDS:
            for w, h in C_SHAPES:
                for _ in range(C_REPLICAS):
                    fr = rng.integers(0, 8, 4)
                    mv = (_small_mv(rng, int(fr[0]), int(fr[1])), _small_mv(rng, int(fr[2]), int(fr[3])))
                    pus.append(Pu(w, h, kind, mv, entry, note=f"[C: entry {e}]"))
    pus = [pus[i] for i in rng.permutation(len(pus))]
    lists = _pack_pus(f"C chroma {chroma} {bd} bit", chroma, bd, pus, seed=13, width=256)
    assert len(lists) == 1
    return lists


# ------------------------------------------------------------------------------------------------------------- family D ----
@functools.lru_cache(maxsize=4)
def build_d(chroma, bd):
    """1 .. 8 PUs of 8x8 and of 8x4 in a 64x8 picture (luma / chroma job counts = 1, 2, 3, 0 mod 4: dead quarters of the last wave),
    one PU alone as uni and as bi, four PUs in each of the 16 uni / bi patterns"""
    rng = np.random.default_rng(4000 + 16 * chroma + bd)
    p = params(64, 8, chroma, bd)
    rec = F.Recorder(p)
    lists = []
    for h in (8, 4):
        plans = [(n, None) for n in range(1, 9)] + [(4, pat) for pat in range(16)] + [(1, 0), (1, 1)]
        for n, pat in plans:
            if pat is None:
                pat = int(rng.integers(1 << n))
            pus = []
            for i in range(n):
                fr = rng.integers(0, 8, 4)
                mv = (_small_mv(rng, int(fr[0]), int(fr[1])), _small_mv(rng, int(fr[2]), int(fr[3])))
                kind = "bi" if (pat >> i) & 1 else ("uni0", "uni1")[int(rng.integers(2))] if n > 1 else "uni0"
                pus.append(Pu(8, h, kind, mv, None, f"[D: {n} PUs pattern {pat:0{n}b}]", 8 * i, 0))
            lists.append(record(f"D 8x{h} chroma {chroma} {bd} bit {n} PUs pattern {pat:0{n}b}", p, pus, [], seed=14, rec=rec))
    rec.close()
    return lists


def d_patterns(lists):
    """{(PU height, number of PUs, uni / bi pattern as bits)}"""
    return {(dl.pus[0].h, len(dl.pus), sum((u.kind == "bi") << i for i, u in enumerate(dl.pus))) for dl in lists}


# ------------------------------------------------------------------------------------------------------------- family E ----
@functools.lru_cache(maxsize=4)
def dct_matrix(n):
    """n-point basis: every (32/n)-th row of the 32-point matrix built from the 32 constants (as ohk_init_residual does)"""
    m = np.zeros((32, 32), np.int64)
    for k in range(32):
        for i in range(32):
            a = (k * (2 * i + 1)) & 127
            if a > 64:
                a = 128 - a
            m[k, i] = 64 if k == 0 else (0 if a == 32 else (_DCT_C[a] if a < 32 else -_DCT_C[64 - a]))
    m = m[::32 // n, :n].copy()
    m.setflags(write=False)
    return m


def idct_model(c, bd, dst=False, clip1=True, clip2=True):
    """(m1) numpy inverse transform of an n x n int16 block: columns (shift 7), clip to int16, rows (shift 20 - bd), clip to int16.
    Returns (residual as int64, hits of the first clip, hits of the second clip); a switched-off clip passes its values through."""
    m = _DST7 if dst else dct_matrix(c.shape[0])
    t = (m.T @ c.astype(np.int64) + 64) >> 7                  # t[i, col] = sum_k m[k, i] c[k, col]
    hits1 = int(np.count_nonzero((t < -32768) | (t > 32767)))
    if clip1:
        t = np.clip(t, -32768, 32767)
    r = (t @ m + (1 << (19 - bd))) >> (20 - bd)               # r[row, i] = sum_k t[row, k] m[k, i]
    hits2 = int(np.count_nonzero((r < -32768) | (r > 32767)))
    if clip2:
        r = np.clip(r, -32768, 32767)
    return r, hits1, hits2


def wrap16(a):
    return ((np.asarray(a, np.int64) + 32768) & 0xffff) - 32768


def e_blocks(n, bd, dst=False):
    """[(recipe, n x n int16 block)] of one (bit depth, size) cell: e1 dense, e2 sign-aligned, e3 single, e4 two corners"""
    rng = np.random.default_rng(5000 + 64 * bd + n + (1 if dst else 0))
    m = _DST7 if dst else dct_matrix(n)
    out = [(f"e1 dense uniform int16 block {k}", rng.integers(-32768, 32768, size=(n, n)).astype(np.int16)) for k in range(E_DENSE)]
    sgn = np.where(m < 0, -1, 1)                              # zeros of the basis taken as +
    for i0 in range(4):
        for j0 in range(4):
            out.append((f"e2 sign-aligned +-32767 for output ({i0}, {j0})", (32767 * np.outer(sgn[:, i0], sgn[:, j0])).astype(np.int16)))
    edges = [e for e in E_EDGES if e < n]
    for r in edges:
        for c in edges:
            for v in (32767, -32767, -32768):
                b = np.zeros((n, n), np.int16)
                b[r, c] = v
                out.append((f"e3 single coefficient {v} at row {r} column {c}", b))
    for ia, a in enumerate(edges):
        for b_ in edges[ia + 1:]:
            for anti in (0, 1):
                b = np.zeros((n, n), np.int16)
                (r0, c0), (r1, c1) = ((a, a), (b_, b_)) if not anti else ((a, b_), (b_, a))
                b[r0, c0], b[r1, c1] = 32767, -32768
                out.append((f"e4 coefficients 32767 at ({r0}, {c0}) and -32768 at ({r1}, {c1})", b))
    return out


def e_items(chroma, bd):
    """every block of the family for one format as Tu records (unplaced), each once inter and once as an intra residual"""
    tus, k = [], 0

    def both(log2, kind, flags, coeffs, recipe, luma_only=False):
        nonlocal k
        for intra in (False, True):
            n = 1 << log2
            c = 0 if luma_only or not chroma or (chroma != 3 and n == 32) else k % 3
            k += 1
            tus.append(Tu(log2, kind, flags, coeffs, recipe, c=c, intra=intra))
    for log2 in (2, 3, 4, 5):
        n = 1 << log2
        blocks = e_blocks(n, bd)
        for recipe, b in blocks:
            both(log2, F.TU_IDCT, 0, b, recipe)
        if n == 4:
            for recipe, b in e_blocks(4, bd, dst=True):
                both(2, F.TU_DST4, 0, b, recipe + " (DST basis)", luma_only=True)
        dense = blocks[:4]
        for kind in (F.TU_SKIP, F.TU_BYPASS):
            for flags, what in ((0, "plain"), (F.TUF_RDPCM, "horizontal rdpcm"), (F.TUF_RDPCM | F.TUF_RDPCM_VER, "vertical rdpcm")):
                for recipe, b in dense:
                    both(log2, kind, flags, b, f"{recipe}, {what}")
        if n == 4:
            for flags, what in ((F.TUF_ROTATE, "rotated"), (F.TUF_ROTATE | F.TUF_RDPCM, "rotated, horizontal rdpcm")):
                for recipe, b in dense:
                    both(2, F.TU_SKIP, flags, b, f"{recipe}, {what}")
    return tus


E_PARTS = 12                                                  # the blocks of a format are dealt to this many test cases


@functools.lru_cache(maxsize=32)
def build_e(chroma, bd, part=None, pinned_by=None):
    """the blocks shuffled, dealt to E_PARTS parts (part=None: all of them) and packed plane by plane into pictures"""
    if part is None:
        return [dl for k in range(E_PARTS) for dl in build_e(chroma, bd, k, pinned_by)]
    rng = np.random.default_rng(6000 + 16 * chroma + bd)
    tus = e_items(chroma, bd)
    queue = [tus[i] for i in rng.permutation(len(tus))[part::E_PARTS]]
    lists = []
    p_full = params(MAX_DIM, MAX_DIM, chroma, bd)
    while queue:
        here, rest = [], []
        for c in range(F.n_planes(p_full)):
            mine = [t for t in queue if t.c == c]
            pw, ph = F.plane_dims(p_full, c)
            placed, left = shelf_pack([(1 << t.log2, 1 << t.log2) for t in mine], pw, ph)
            for i in sorted(placed):
                mine[i].x, mine[i].y = placed[i]
                here.append(mine[i])
            rest += [mine[i] for i in sorted(left)]
        order = {id(t): i for i, t in enumerate(queue)}
        here.sort(key=lambda t: order[id(t)])                 # the shuffled order: a wave of residual_kernel mixes kinds and recipes
        queue = sorted(rest, key=lambda t: order[id(t)])
        height = max(((t.y + (1 << t.log2)) << F.vshift(p_full, t.c)) for t in here)
        lists.append(record(f"E chroma {chroma} {bd} bit part {part} picture {len(lists)}", params(MAX_DIM, (height + 63) // 64 * 64, chroma, bd),
                            [], here, seed=15, pinned_by=pinned_by))
    return lists


# ------------------------------------------------------------------------------------------------------------- model m2 ----
def expected_pu(ref, p, u, pics):
    """(m2) one PU composed from the REFERENCE's slots: the window of each list is gathered with clamped coordinates (what
    emulated_edge_mc produces), list 0 of a bi PU goes through variant 0 (put) into an int16 buffer, the rest through variant 1-4.
    Chroma vector and fraction as in hevc.c:1807-1813.  Returns [(plane, x, y, samples)]."""
    bd = p.bit_depth
    bpp = 1 if bd == 8 else 2
    out = []
    for c in range(F.n_planes(p)):
        hs, vs = F.hshift(p, c), F.vshift(p, c)
        epel = int(c > 0)
        before, after = (1, 2) if epel else (3, 4)
        bx, by, bw, bh = u.x >> hs, u.y >> vs, u.w >> hs, u.h >> vs
        lists = [l for l in (0, 1) if u.refs[l] >= 0]
        wins, fr = {}, {}
        for l in lists:
            mvx, mvy = u.mv[l]
            if c == 0:
                fr[l], ix, iy = (mvx & 3, mvy & 3), mvx >> 2, mvy >> 2
            else:
                fr[l] = ((mvx & ((1 << (2 + hs)) - 1)) << (1 - hs), (mvy & ((1 << (2 + vs)) - 1)) << (1 - vs))
                ix, iy = mvx >> (2 + hs), mvy >> (2 + vs)
            plane = pics[u.refs[l]].visible(c)
            ys = np.clip(np.arange(by + iy - before, by + iy + bh + after), 0, plane.shape[0] - 1)
            xs = np.clip(np.arange(bx + ix - before, bx + ix + bw + after), 0, plane.shape[1] - 1)
            wins[l] = np.ascontiguousarray(plane[np.ix_(ys, xs)])
        def src(l):
            return off_u8p(wins[l], before * wins[l].strides[0] + before * bpp), wins[l].strides[0]
        dst = np.zeros((bh, bw), pix_dtype(bd))
        denom = u.wt[1 if c else 0] if u.wt else 0
        w = (u.wt[2], u.wt[4]) if u.wt else (0, 0)
        o = (u.wt[3], u.wt[5]) if u.wt else (0, 0)
        if len(lists) == 2:
            tmp = np.zeros((bh, 64), np.int16)
            s0, st0 = src(0)
            ref.ref_mc(bd, epel, 0, C.cast(i16p(tmp), C.POINTER(C.c_uint8)), 64, s0, st0, None, 0, bh, 0, 0, 0, 0, 0, fr[0][0], fr[0][1], bw)
            s1, st1 = src(1)
            ref.ref_mc(bd, epel, 4 if u.wt else 2, u8p(dst), dst.strides[0], s1, st1, i16p(tmp), 64, bh, denom, w[0], w[1], o[0], o[1],
                       fr[1][0], fr[1][1], bw)
        else:
            l = lists[0]
            s, st = src(l)
            ref.ref_mc(bd, epel, 3 if u.wt else 1, u8p(dst), dst.strides[0], s, st, None, 0, bh, denom, w[l], 0, o[l], 0, fr[l][0], fr[l][1], bw)
        out.append((c, bx, by, dst))
    return out
