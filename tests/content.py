"""Test content with structure.  The picture-level tests fill their pictures with uniform noise by default; on noise the luma
deblocking decision d0 + d3 < beta almost never holds, so most of the filter never runs.  The generators here make low-activity
pictures, and STRUCTURED_CASES names the work lists that go with them; tests/test_structured_content.py keeps both honest from
the oracle's decision counters (oh_or_counters), tests/test_gpu_structured.py runs them through the engine."""
import numpy as np

from openhevc_amd import frame as F


def _sine_base(p, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (np.sin(xx / 37.0) + np.cos(yy / 23.0)) * (40 << (p.bit_depth - 8)) + (128 << (p.bit_depth - 8))


def smooth_picture(p, rng):
    """low-activity content so that deblocking decisions and SAO categories all occur"""
    hp = F.HostPic(p)
    for c, pl in enumerate(hp.planes):
        h, w = pl.shape
        base = _sine_base(p, h, w)
        blocks = rng.integers(-6, 7, size=(h // 8 + 1, w // 8 + 1)) * (1 << (p.bit_depth - 8))
        noise = rng.integers(-2, 3, size=(h, w)) * (1 << (p.bit_depth - 8))
        v = base + np.kron(blocks, np.ones((8, 8)))[:h, :w] + noise
        pl[:] = np.clip(v, 0, (1 << p.bit_depth) - 1).astype(pl.dtype)
    return hp


ZONE_JITTER = (0, 1, 3)             # x 2^(bd - 8), per vertical zone
ZONE_SHARE = (0.45, 0.35, 0.20)     # of the plane's width: the textured zone that leaves the filter off is the narrowest


def zoned_picture(p, rng):
    """the sine base of smooth_picture plus a step of +-6 * 2^(bd - 8) per 16x16 block, in three vertical zones with per-sample
    jitter of amplitude 0, 1 and 3 (* 2^(bd - 8)): flat steps make the strong filter possible, mild texture gives the normal
    filter, the third zone leaves it off.  Two plateaus, one clipped at 0 and one at the largest sample value, are there for
    the saturation in the filters' sample clip; each covers a fifth of the width and a third of the height and straddles two
    zones, so no zone is swallowed."""
    hp = F.HostPic(p)
    sc, mx = 1 << (p.bit_depth - 8), (1 << p.bit_depth) - 1
    for c, pl in enumerate(hp.planes):
        h, w = pl.shape
        vw = F.plane_dims(p, c)[0]                                      # the zones divide the visible width
        steps = (2 * rng.integers(0, 2, size=(h // 16 + 1, w // 16 + 1)) - 1) * 6 * sc
        v = _sine_base(p, h, w) + np.kron(steps, np.ones((16, 16)))[:h, :w]
        x0 = 0
        for amp, share in zip(ZONE_JITTER, ZONE_SHARE):
            x1 = w if amp == ZONE_JITTER[-1] else x0 + int(round(vw * share))
            if amp:
                v[:, x0:x1] += rng.integers(-amp, amp + 1, size=(h, x1 - x0)) * sc
            x0 = x1
        pw, ph = max(4, vw // 5), max(4, h // 3)
        for level, px, py in ((0, int(vw * 0.45) - pw // 2, 0), (mx, int(vw * 0.80) - pw // 2, h - ph)):
            r = v[py:py + ph, px:px + pw]
            r += level - np.round(r.mean())                               # about half of the plateau saturates
        pl[:] = np.clip(v, 0, mx).astype(pl.dtype)
    return hp


PCM = {"pcm_loop_filter_disable": 1, "transquant_bypass_enable": 1}
SIS = {"strong_intra_smoothing": 1}

STRUCTURED_CASES = [
    # name, w, h, bd, chroma, log2_ctb, slice_type, picture parameters, generator knobs (coeff_shift / pcm_flat: STRUCTURED_KNOBS)
    ("i8_sis", 416, 240, 8, 1, 6, 0, SIS, {"split_pct": 20, "coeff_shift": 3}),
    ("p8_weighted", 264, 200, 8, 1, 5, 1, {"cb_qp_offset": 2, "cr_qp_offset": -3}, {"weighted_pct": 50}),
    ("b8", 416, 240, 8, 1, 6, 2, {}, {}),
    ("i10_sis", 416, 240, 10, 1, 6, 0, SIS, {"split_pct": 20, "coeff_shift": 3}),
    ("p10_ctb16_offsets", 200, 136, 10, 1, 4, 1, {}, {"vary_deblock_offsets": 1}),
    ("b10_cip", 264, 200, 10, 1, 6, 2, {"constrained_intra_pred": 1}, {"intra_pct": 50}),
    ("i12", 136, 88, 12, 1, 5, 0, {}, {"coeff_shift": 2}),
    ("p12_bs_from_motion", 200, 136, 12, 1, 5, 1, {}, {"bs_from_motion": 1, "intra_pct": 25}),
    ("b12", 136, 88, 12, 1, 5, 2, {}, {}),
    ("b10_444", 136, 88, 10, 3, 5, 2, {}, {}),
    ("i8_mono", 128, 64, 8, 0, 6, 0, {}, {"coeff_shift": 2}),
    ("b8_ctb16_one_row", 96, 16, 8, 1, 4, 2, {}, {"sao_pct": 90, "intra_pct": 30}),
    ("b10_sparse_lists", 264, 200, 10, 1, 5, 2, {}, {"sparse_pct": 100, "scaling_list": 1, "intra_pct": 30, "cbf_pct": 35}),
    ("b8_slices_deblock_off", 264, 200, 8, 1, 4, 2, {}, dict(n_slices=9, sao_pct=80,
                                                            slice_knobs=F.SYNTH_NO_LF_ACROSS_SLICES | F.SYNTH_DEBLOCK_OFF_SLICES)),
    ("b10_tiles", 416, 240, 10, 1, 5, 2, {}, dict(tile_cols=3, tile_rows=2, sao_pct=80,
                                                  slice_knobs=F.SYNTH_NO_LF_ACROSS_TILES | F.SYNTH_SLICE_PER_TILE)),
    ("b8_pcm_bypass", 264, 200, 8, 1, 6, 2, PCM, {"pcm_pct": 20, "bypass_pct": 12, "intra_pct": 30, "qp_base": 34}),
    ("b10_pcm_bypass", 264, 200, 10, 1, 5, 2, PCM, {"pcm_pct": 12, "bypass_pct": 12, "intra_pct": 30}),
    ("b8_422_pcm_bypass", 200, 136, 8, 2, 6, 2, PCM, {"pcm_pct": 12, "bypass_pct": 12, "intra_pct": 30}),
    ("b10_422_pcm_bypass", 200, 136, 10, 2, 5, 2, PCM, {"pcm_pct": 12, "bypass_pct": 12, "intra_pct": 30}),
]
STRUCTURED_IDS = [c[0] for c in STRUCTURED_CASES]
STRUCTURED_SEEDS = (0, 1)
STRUCTURED_KNOBS = {"coeff_shift": 4, "pcm_flat": 1}


def case_named(name):
    return STRUCTURED_CASES[STRUCTURED_IDS.index(name)]


def structured_params(case):
    _, w, h, bd, chroma, lc, _, pic_kw, _ = case
    return F.pic_params(w, h, bit_depth=bd, chroma_format_idc=chroma, log2_ctb_size=lc, **pic_kw)


def structured_picture(case, rec, seed, synth_seed=None):
    """(work list, {id: HostPic}) of one seed of a case from recorder `rec`: references 0 and 1 from zoned_picture, the current
    picture 2 noise (every sample of it must be overwritten).  The list lives until rec's next picture."""
    st, knobs = case[6], case[8]
    p = rec.params
    f = rec.synth(F.synth_params(st, (6000 if synth_seed is None else synth_seed) + seed, **dict(STRUCTURED_KNOBS, **knobs)),
                  2, [0, 1] if st else [])
    rng = np.random.default_rng(seed)
    return f, {0: zoned_picture(p, rng), 1: zoned_picture(p, rng), 2: F.HostPic(p, rng=rng)}
