"""Rate of the light-level pass (oh_pics_light_level) beside the colour conversion (oh_pics_convert_colour) of the same pictures to
linear-light BT.2020 f16 planar with no tone curve — the conversion that does the same stages 0 and 1 per pixel and writes 6 bytes per
pixel on top: 32 pictures of 3840x2160 4:2:0 Main 10, PQ / BT.2020 (matrix 9, limited range, linear chroma), one call each, on
    random content (uniform codes: the histogram spreads over its bins, every workgroup flushes most of them) and
    low-activity content (tests/content.py smooth_picture: neighbouring pixels share a bin, the histogram is concentrated) and
    flat content (one grey per picture: every pixel of a workgroup in one bin, the worst case for atomics on one address).
Device time between two events on the engine's stream around `reps` calls; the two alternate, `rounds` times; the figure is the best
round, the worst is printed.  A light-level call ends with a wait for its results, so its figure includes the clear, the copy of the
results and the host's turn-around between calls; the kernels alone come from a profiler run of its own:

    python tools/light_rate.py [--pictures 32] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o light -- python tools/light_rate.py --reps 10 --rounds 2
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, BD = 3840, 2160, 10


def pictures(F, p, content, n):
    """n pictures derived from one generated picture (generating 32 of this size takes minutes)"""
    from content import smooth_picture
    rng = np.random.default_rng(1)
    base = F.HostPic(p, rng=rng) if content == "random" else smooth_picture(p, rng)
    if content == "flat":
        for c in range(3):
            base.visible(c)[...] = 1 << (BD - 1)
    top = (1 << BD) - 1
    out = []
    for k in range(n):
        hp = F.HostPic(p)
        for c in range(3):
            v = base.visible(c).astype(np.int64)
            hp.visible(c)[...] = (v + 37 * k) & top if content == "random" else np.clip(v + (k % 8) - 4, 0, top)
        out.append(hp)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch

    from openhevc_amd import engine as E
    from openhevc_amd import frame as F
    stream = torch.cuda.current_stream()
    eng = E.Engine(0, stream=stream.cuda_stream)             # on torch's stream: torch events time the engine's launches
    p = F.pic_params(W, H, bit_depth=BD, chroma_format_idc=1)
    lin = E.make_colour(16, 9, out="linear", out_primaries=9, tone="none")
    kw = dict(dtype=torch.float16, matrix=9, full_range=False, chroma="linear")
    pids = [eng.pic_alloc(p) for _ in range(a.pictures)]
    out = None

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for content in ("random", "low_activity", "flat"):
        for pid, hp in zip(pids, pictures(F, p, content, a.pictures)):
            eng.pic_upload(pid, hp)
        eng.sync()
        for norm in ("maxrgb", "luma"):
            def light():
                return eng.pics_light_level(pids, 16, in_primaries=9, norm=norm, matrix=9)

            def colour():
                return eng.pics_convert(pids, "rgb_planar", out=out, colour=lin, **kw)

            lls = light()                                     # warm-up of both kernels; the same tensor is reused
            out = colour()
            torch.cuda.synchronize()
            ms = {"light": [], "colour": []}
            for _ in range(a.rounds):
                ms["light"].append(timed(light))
                ms["colour"].append(timed(colour))
            best = {k: min(v) for k, v in ms.items()}
            hist = sum(ll.hist.astype(np.int64) for ll in lls)
            print(json.dumps({"content": content, "norm": norm, "pictures": a.pictures, "bins_used": int((hist > 0).sum()),
                              "largest_bin_share": round(float(hist.max() / hist.sum()), 3),
                              "peak_nits_9999": round(E.source_peak(16, lls), 1),
                              "light_ms": round(best["light"], 4), "light_ms_worst": round(max(ms["light"]), 4),
                              "colour_ms": round(best["colour"], 4), "colour_ms_worst": round(max(ms["colour"]), 4),
                              "light_Gpixels_per_s": round(a.pictures * W * H / (best["light"] * 1e-3) / 1e9, 1),
                              "ratio": round(best["light"] / best["colour"], 3)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
