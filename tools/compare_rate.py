"""Rate of the picture comparison (oh_pics_compare) with and without OH_CMP_SSIM, beside the checksum pass of oh_pics_hash over the
same pictures in the same run — existing code that reads every byte of one picture at HBM rate, where the comparison reads two:
64 pairs of 3840x2160 4:2:0 Main 10 (128 different pictures, 3.2 GB of packed planes: more than the Infinity Cache holds), one call
each, on
    random content (b independent of a: every sample differs, every workgroup issues its atomics) and
    equal content (b a copy of a in memory of its own: no workgroup has a difference to add).
Host wall time per call around `reps` calls — each of the three ends with a wait for the engine stream, so the figure holds the clear
and the copy of the results and the host's turn-around as well; the three alternate, `rounds` times; the figure is the best round, the
worst is printed.  The kernels alone come from a profiler run of its own:

    python tools/compare_rate.py [--pairs 64] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o compare -- python tools/compare_rate.py --reps 5 --rounds 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BD = 3840, 2160, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from openhevc_amd import engine as E
    from openhevc_amd import frame as F
    eng = E.Engine(0)
    p = F.pic_params(W, H, bit_depth=BD, chroma_format_idc=1)
    n, top = a.pairs, (1 << BD) - 1
    ids_a = [eng.pic_alloc(p) for _ in range(n)]
    ids_b = [eng.pic_alloc(p) for _ in range(n)]
    rng = np.random.default_rng(1)
    base = [F.HostPic(p, rng=rng) for _ in range(2)]
    nbytes = 2 * n * sum(base[0].visible(c).nbytes for c in range(3))     # what one call of either kind reads

    def derived(src, k):
        hp = F.HostPic(p)
        for c in range(3):
            hp.visible(c)[...] = (src.visible(c) + np.uint16(37 * k)) & top
        return hp

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        return (time.perf_counter() - t0) / a.reps * 1e3

    for content in ("random", "equal"):
        for k in range(n):
            eng.pic_upload(ids_a[k], derived(base[0], k))
            eng.pic_upload(ids_b[k], derived(base[content == "random"], k))
        eng.sync()
        calls = {"compare": lambda: eng.pics_compare(ids_a, ids_b, ssim=False),
                 "compare_ssim": lambda: eng.pics_compare(ids_a, ids_b, ssim=True),
                 "checksum": lambda: eng.pics_hash(ids_a + ids_b, 2)}
        res = calls["compare_ssim"]()                         # warm-up: code objects, staging and device buffers
        calls["compare"]()
        calls["checksum"]()
        ms = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                ms[k].append(timed(fn))
        best = {k: min(v) for k, v in ms.items()}
        y = res[0].plane[0]
        out = {"content": content, "pairs": n, "geometry": f"{W}x{H} {BD} bit 4:2:0", "bytes_read": nbytes,
               "luma_psnr_pair0": round(y.psnr, 3) if y.differing else None, "luma_ssim_pair0": round(y.ssim, 6), "luma_differing_pair0": y.differing}
        for k in calls:
            out[k + "_ms"] = round(best[k], 4)
            out[k + "_ms_worst"] = round(max(ms[k]), 4)
            out[k + "_GBps"] = round(nbytes / (best[k] * 1e-3) / 1e9, 1)
        out["compare_to_checksum_rate"] = round(best["checksum"] / best["compare"], 3)
        out["compare_ssim_to_checksum_rate"] = round(best["checksum"] / best["compare_ssim"], 3)
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
