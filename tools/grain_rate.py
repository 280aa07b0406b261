"""Rate of oh_pics_grain on 32 pictures of 3840x2160 4:2:0 per call, at 10 and at 8 bit, beside oh_pics_reformat to the same depth and
format on the same pictures in the same run (a copy of the coded planes: time per destination byte relative to the copy).

  uniform     one entry for every intensity of every plane (one pattern in use), on noise
  intervals   ten intervals per plane, each with its own sigma and cut-offs (ten patterns a plane), on noise: neighbouring blocks differ
  luma        the uniform grain on luma alone; both chroma planes are copied by the same kernel

Host wall time per call around `reps` calls and a wait for the engine stream; case and copy alternate, `rounds` times; the figures are
the median and the range of the rounds.

    python tools/grain_rate.py [--pictures 32] [--reps 3] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160


def planes(bd, w, h):
    """bytes of the coded planes of one 4:2:0 picture"""
    return w * h * 3 // 2 * (2 if bd > 8 else 1)


def run(a):
    import numpy as np
    import torch

    from openhevc_amd import engine as E
    eng = E.Engine(0)
    n = a.pictures
    g = torch.Generator(device="cuda:0").manual_seed(22)
    yuv = torch.randint(0, 1024, (n, H * 3 // 2, W), dtype=torch.int32, device="cuda:0", generator=g)
    # noise around block means that spread over the intervals: a random level per 8 x 8 luma block, +- 32 of noise
    level = torch.randint(64, 960, (n, H * 3 // 2 // 8, W // 8), dtype=torch.int32, device="cuda:0", generator=g)
    yuv = (level.repeat_interleave(8, 1).repeat_interleave(8, 2) + (yuv & 63) - 32).clamp_(0, 1023)
    p10 = eng.pics_import(yuv.to(torch.int16).view(torch.uint16), "planar", bit_depth=10, chroma_format_idc=1)[0]
    sets = {10: p10, 8: eng.pics_reformat(p10, bit_depth=8)}
    eng.sync()
    del yuv, level

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        eng.sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    def stats(v):
        return round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)

    ten = np.zeros((3, 256), dtype=np.uint32)
    for c in range(3):
        for k in range(10):
            ten[c, 26 * k:26 * (k + 1) if k < 9 else 256] = (20 + 10 * k) | (2 + (k + 4 * c) % 13) << 8 | (14 - (2 * k + c) % 13) << 12
    cases = {"uniform": E.make_grain(40, 8, 8, log2_scale=2), "intervals": E.Grain(ten, 7, 0, 2),
             "luma": E.make_grain(40, 8, 8, log2_scale=2, planes=1)}
    for bd in (10, 8):
        src = sets[bd]
        sp = eng._pic_params(src[0])
        cp, dst = eng._alloc_like(sp, n), eng._alloc_like(sp, n)
        for name, grain in cases.items():
            def case():
                return eng.pics_grain(src, grain, 1000, out=dst)

            def copy():
                return eng.pics_reformat(src, out=cp)

            case()
            copy()
            eng.sync()
            ms, cms = [], []
            for _ in range(a.rounds):
                ms.append(timed(case))
                cms.append(timed(copy))
            med, lo, hi = stats(ms)
            cmed, clo, chi = stats(cms)
            print(json.dumps({"case": name, "bits": bd, "pictures": n, "image": [W, H], "ms_median": med, "ms_min": lo, "ms_max": hi,
                              "copy_ms_median": cmed, "copy_ms_min": clo, "copy_ms_max": chi, "dst_bytes": n * planes(bd, W, H),
                              "GB_per_s_written": round(n * planes(bd, W, H) / med / 1e6, 1),
                              "time_per_dst_byte_to_copy": round(med / cmed, 2)}), flush=True)
        for pid in cp + dst:
            eng.pic_free(pid)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
