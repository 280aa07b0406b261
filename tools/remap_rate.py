"""Rate of oh_pics_colour_remap on 32 pictures of 3840x2160 4:4:4 per call, at 10 -> 10, 10 -> 8, 8 -> 8 and 12 -> 12 bit, on noise and
on a smooth ramp (the bank conflicts of the LDS gathers depend on the content), beside oh_pics_reformat of the same sources to their
own depth and format in the same run (a copy of the coded planes): time per destination byte relative to the copy.

  full        random tables, a full matrix with negative entries
  identity    the same tables, the identity matrix
  lut         the same tables and a diagonal matrix, through Remap.luts() and oh_pics_lut: the per-plane form of the same work

Host wall time per call around `reps` calls and a wait for the engine stream; case and copy alternate, `rounds` times; the figures are
the median and the range of the rounds.

    python tools/remap_rate.py [--pictures 32] [--reps 3] [--rounds 5] [--pairs 10:10,10:8,8:8,12:12]
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
    """bytes of the coded planes of one 4:4:4 picture"""
    return w * h * 3 * (2 if bd > 8 else 1)


def run(a):
    import numpy as np
    import torch

    from openhevc_amd import engine as E
    eng = E.Engine(0)
    n = a.pictures
    g = torch.Generator(device="cuda:0").manual_seed(23)
    rng = np.random.default_rng(23)

    def sources(bd, kind):
        if kind == "noise":
            yuv = torch.randint(0, 1 << bd, (n, H * 3, W), dtype=torch.int32, device="cuda:0", generator=g)
        else:                                                   # a diagonal ramp of one code value every four samples, its own phase per plane row
            x = torch.arange(W, dtype=torch.int32, device="cuda:0")[None, None, :]
            y = torch.arange(H * 3, dtype=torch.int32, device="cuda:0")[None, :, None]
            i = torch.arange(n, dtype=torch.int32, device="cuda:0")[:, None, None]
            yuv = ((x + y + 37 * i) >> 2) & ((1 << bd) - 1)
        t = yuv.to(torch.int16).view(torch.uint16) if bd > 8 else yuv.to(torch.uint8)
        return eng.pics_import(t.contiguous(), "planar", bit_depth=bd, chroma_format_idc=3)[0]

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        eng.sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    def stats(v):
        return round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)

    for bi, bo in a.pairs:
        pre = rng.integers(0, 1 << bo, (3, 1 << bi)).astype(np.uint16)
        post = rng.integers(0, 1 << bo, (3, 1 << bo)).astype(np.uint16)
        d = 10
        full = np.array([[900, -200, 150], [-120, 1100, 60], [40, -300, 1000]])
        remaps = {"full": E.Remap(pre, full, d, post, bi, bo), "identity": E.Remap(pre, np.eye(3, dtype=np.int64) << d, d, post, bi, bo)}
        luts = list(E.Remap(pre, np.diag(np.diag(full)), d, post, bi, bo).luts())
        for kind in ("noise", "ramp"):
            src = sources(bd=bi, kind=kind)
            eng.sync()
            sp = eng._pic_params(src[0])
            dp = type(sp).from_buffer_copy(sp)
            dp.bit_depth = bo
            cp, dst = eng._alloc_like(sp, n), eng._alloc_like(dp, n)
            cases = {name: (lambda r=r: eng.pics_colour_remap(src, r, out=dst)) for name, r in remaps.items()}
            cases["lut"] = lambda: eng.pics_lut(src, luts, out=dst)

            def copy():
                return eng.pics_reformat(src, out=cp)

            for name, case in cases.items():
                case()
                copy()
                eng.sync()
                ms, cms = [], []
                for _ in range(a.rounds):
                    ms.append(timed(case))
                    cms.append(timed(copy))
                med, lo, hi = stats(ms)
                cmed, clo, chi = stats(cms)
                db, cb = n * planes(bo, W, H), n * planes(bi, W, H)
                print(json.dumps({"case": name, "content": kind, "bits": [bi, bo], "pictures": n, "image": [W, H], "ms_median": med, "ms_min": lo,
                                  "ms_max": hi, "copy_ms_median": cmed, "copy_ms_min": clo, "copy_ms_max": chi, "dst_bytes": db,
                                  "copy_dst_bytes": cb, "GB_per_s_written": round(db / med / 1e6, 1),
                                  "time_per_dst_byte_to_copy": round(med / db / (cmed / cb), 2),
                                  "time_per_dst_byte_to_copy_min": round(lo / db / (chi / cb), 2),
                                  "time_per_dst_byte_to_copy_max": round(hi / db / (clo / cb), 2)}), flush=True)
            for pid in cp + dst + src:
                eng.pic_free(pid)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=lambda s: [tuple(int(v) for v in p.split(":")) for p in s.split(",")],
                    default=[(10, 10), (10, 8), (8, 8), (12, 12)])
    run(ap.parse_args())


if __name__ == "__main__":
    main()
