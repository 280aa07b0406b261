"""Rate of the picture import (oh_pics_import) beside oh_pics_convert of the same format on the same pictures in the same run — the
conversion is existing code that moves the same bytes in the other direction: 32 pictures of 3840x2160 4:2:0 per call, the cases
P010 and I420 u8 into Main 10, NV12 into 8 bit, and RGB u8 interleaved, RGB f16 planar and RGB f32 planar into Main 10 (BT.709,
limited range, linear chroma, window = the whole picture).  The images a case imports are what its conversion wrote.  Host wall
time per call around `reps` calls and a wait for the engine stream; the two alternate, `rounds` times; the figure is the best
round.  The kernels alone come from a profiler run of its own:

    python tools/import_rate.py [--pictures 32] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o import -- python tools/import_rate.py --reps 10 --rounds 2
    python tools/import_rate.py --summarize OUT          kernel times of that run (its *kernel_stats.csv): import / convert per case
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
# (label, picture bit depth, format, dtype name, import kernel as the profiler names it, convert kernel, margin the issue expects)
CASES = [("P010 into Main 10", 10, "semiplanar", "uint16", "import_yuv_kernel<unsigned short, unsigned short, 1>",
          "convert_yuv_kernel<unsigned short, 1, 1>", 1.25),
         ("I420 u8 into Main 10", 10, "planar", "uint8", "import_yuv_kernel<unsigned char, unsigned short, 0>",
          "convert_yuv_kernel<unsigned short, 0, 0>", 1.25),
         ("NV12 into 8 bit", 8, "semiplanar", "uint8", "import_yuv_kernel<unsigned char, unsigned char, 1>",
          "convert_yuv_kernel<unsigned char, 0, 1>", 1.25),
         ("RGB u8 into Main 10", 10, "rgb", "uint8", "import_rgb_kernel<0, unsigned short, 3>", "convert_rgb_kernel<unsigned short, 0, 3>", 1.5),
         ("RGB f16 planar into Main 10", 10, "rgb_planar", "float16", "import_rgb_kernel<2, unsigned short, 2>",
          "convert_rgb_kernel<unsigned short, 2, 2>", 1.5),
         ("RGB f32 planar into Main 10", 10, "rgb_planar", "float32", "import_rgb_kernel<3, unsigned short, 2>",
          "convert_rgb_kernel<unsigned short, 3, 2>", 1.5)]


def call_bytes(bd, fmt, dtype, n):
    """bytes one call of either kind moves: the three planes of every picture and its image"""
    bps = 2 if bd > 8 else 1
    planes = W * H * 3 // 2 * bps
    image = (W * H * 3 // 2 if fmt in ("planar", "semiplanar") else W * H * 3) * {"uint8": 1, "uint16": 2, "float16": 2, "float32": 4}[dtype]
    return n * (planes + image)


def run(a):
    import torch

    from openhevc_amd.engine import Engine
    eng = Engine(0)
    n = a.pictures
    sets = {}
    for bd in (10, 8):
        # the source pictures are imports themselves: random RGB made on the device
        g = torch.Generator(device="cuda:0").manual_seed(bd)
        rgb = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda:0", generator=g)
        src, _ = eng.pics_import(rgb, "rgb", bit_depth=bd, chroma_format_idc=1)
        dst = [eng.pic_alloc(eng._pic_params(src[0])) for _ in range(n)]
        sets[bd] = (src, dst)
        del rgb
    eng.sync()

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        eng.sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    for label, bd, fmt, dt, _, _, margin in CASES:
        src, dst = sets[bd]
        kw = dict(matrix=1, full_range=False, chroma="linear")
        img = eng.pics_convert(src, fmt, dtype=getattr(torch, dt), **kw)     # warm-up; the tensor is reused
        eng.pics_import(img, fmt, out=dst, **kw)
        eng.sync()
        if fmt in ("planar", "semiplanar") and (dt == "uint16" or bd == 8):  # the stored samples come back exactly
            assert all(c.plane[k].differing == 0 for c in eng.pics_compare(src[:2], dst[:2], ssim=False) for k in range(3))
        calls = {"convert": lambda: eng.pics_convert(src, fmt, dtype=getattr(torch, dt), out=img, **kw),
                 "import": lambda: eng.pics_import(img, fmt, out=dst, **kw)}
        ms = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                ms[k].append(timed(fn))
        nb = call_bytes(bd, fmt, dt, n)
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps({"case": label, "pictures": n, "bytes": nb, "import_ms": round(best["import"], 4),
                          "import_ms_worst": round(max(ms["import"]), 4), "convert_ms": round(best["convert"], 4),
                          "convert_ms_worst": round(max(ms["convert"]), 4), "import_TBps": round(nb / (best["import"] * 1e-3) / 1e12, 2),
                          "import_to_convert": round(best["import"] / best["convert"], 3), "expected_within": margin}), flush=True)
        del img
    eng.close()


def summarize(a):
    """kernel times of a rocprofv3 --kernel-trace --stats run of this tool: each case's import kernel beside its convert kernel, medians
    over the dispatches of the trace"""
    paths = sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {a.summarize}")
    us = {}
    for r in csv.DictReader(open(paths[-1])):
        us.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)

    def find(kernel):
        for name, v in us.items():
            if kernel + "(" in name:
                v = sorted(v)
                return len(v), v[len(v) // 2], v[0]
        return None
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {a.pictures} pictures {W}x{H} 4:2:0 per call; bytes = planes + images")
    print(f"# {'case':28s} {'calls':>5s} {'import med us':>13s} {'min us':>8s} {'convert med us':>14s} {'min us':>8s} {'MB/call':>8s} "
          f"{'TB/s':>5s} {'ratio med':>9s} {'ratio min':>9s} {'within':>6s}")
    for label, bd, fmt, dt, ik, ck, margin in CASES:
        i, c = find(ik), find(ck)
        if not i or not c:
            continue
        nb = call_bytes(bd, fmt, dt, a.pictures)
        print(f"  {label:28s} {i[0]:5d} {i[1]:13.1f} {i[2]:8.1f} {c[1]:14.1f} {c[2]:8.1f} {nb / 1e6:8.1f} {nb / (i[1] * 1e-6) / 1e12:5.2f} "
              f"{i[1] / c[1]:9.3f} {i[2] / c[2]:9.3f} {margin:6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--summarize", metavar="DIR", help="read the rocprofv3 --stats output under DIR instead of running")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)


if __name__ == "__main__":
    main()
