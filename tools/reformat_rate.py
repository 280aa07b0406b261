"""Rate of the picture reformatting (oh_pics_reformat) beside oh_pics_convert to OH_CONV_PLANAR / OH_CONV_NATIVE of the same source
pictures in the same run — the conversion is existing code that reads the planes and writes the same bytes, in effect a copy: 32
pictures of 3840x2160 per call, the cases
  (a) 4:2:0 10 bit -> 4:2:0 10 bit, a copy
  (b) 4:2:0 10 bit -> 4:2:0 8 bit, dither
  (c) 4:2:0 10 bit -> 4:4:4 10 bit, linear
  (d) 4:4:4 10 bit -> 4:2:0 10 bit, linear
  (e) 4:4:4 12 bit -> 4:2:0 8 bit, linear, dither
bytes of a call: the source planes read and the destination planes written; of the conversion: the source planes read, the image written.
Host wall time per call around `reps` calls and a wait for the engine stream; reformat and conversion alternate, `rounds` times; the
figures are the median and the best round.  The kernels alone come from a profiler run of its own, without counters:

    python tools/reformat_rate.py [--pictures 32] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o reformat -- python tools/reformat_rate.py --reps 10 --rounds 2
    python tools/reformat_rate.py --summarize OUT --reps 10 --rounds 2    kernel times of that run (its *kernel_trace.csv) per case; the
                                                                          cases are told apart by their order, so --reps and --rounds
                                                                          must be the run's
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160


def planes(bd, cf):
    """bytes of the coded planes of one picture"""
    return W * H * {0: 2, 1: 3, 2: 4, 3: 6}[cf] // 2 * (2 if bd > 8 else 1)


# (key, label, source (bit depth, chroma format), destination, keywords of Engine.pics_reformat, margin the issue expects)
CASES = [("a", "4:2:0 10 bit, a copy", (10, 1), (10, 1), {}, 1.25),
         ("b", "4:2:0 10 -> 8 bit, dither", (10, 1), (8, 1), {"depth": "dither"}, 1.25),
         ("c", "10 bit 4:2:0 -> 4:4:4, linear", (10, 1), (10, 3), {"up": "linear"}, 1.5),
         ("d", "10 bit 4:4:4 -> 4:2:0, linear", (10, 3), (10, 1), {"down": "linear"}, 1.5),
         ("e", "4:4:4 12 bit -> 4:2:0 8 bit, linear, dither", (12, 3), (8, 1), {"down": "linear", "depth": "dither"}, 1.5)]
SETUP_CALLS = 2                                             # reformat calls that make the 4:4:4 sources, in front of the cases


def run(a):
    import torch

    from openhevc_amd.engine import Engine
    eng = Engine(0)
    n = a.pictures
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(12)
    yuv = torch.randint(0, 1024, (n, H * 3 // 2, W), dtype=torch.int16, device=dev, generator=g).view(torch.uint16)
    main10, _ = eng.pics_import(yuv, "planar", bit_depth=10, chroma_format_idc=1)
    del yuv
    srcs = {(10, 1): main10}
    srcs[(10, 3)] = eng.pics_reformat(main10, chroma_format_idc=3)          # SETUP_CALLS
    srcs[(12, 3)] = eng.pics_reformat(srcs[(10, 3)], bit_depth=12)
    eng.sync()
    dsts, imgs = {}, {}
    for key, label, s, d, kw, margin in CASES:
        src = srcs[s]
        if d not in dsts:
            dsts[d] = eng.pics_reformat(src, bit_depth=d[0], chroma_format_idc=d[1], **kw)      # warm-up, allocates
        else:
            eng.pics_reformat(src, out=dsts[d], **kw)
        dst = dsts[d]
        if s not in imgs:
            imgs[s] = eng.pics_convert(src, "planar")       # warm-up; the tensor is reused
        else:
            eng.pics_convert(src, "planar", out=imgs[s])
        img = imgs[s]
        eng.sync()
        if key == "a":                                      # same depth and format is a copy
            assert all(c.plane[k].differing == 0 for c in eng.pics_compare(src[:2], dst[:2], ssim=False) for k in range(3))

        def reformat():
            eng.pics_reformat(src, out=dst, **kw)

        def convert():
            eng.pics_convert(src, "planar", out=img)

        def timed(fn):
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            eng.sync()
            return (time.perf_counter() - t0) / a.reps * 1e3

        ms = {"reformat": [], "convert": []}
        for _ in range(a.rounds):
            ms["reformat"].append(timed(reformat))
            ms["convert"].append(timed(convert))
        med = {k: statistics.median(v) for k, v in ms.items()}
        best = {k: min(v) for k, v in ms.items()}
        nbytes, cbytes = planes(*s) + planes(*d), 2 * planes(*s)
        ratio = (med["reformat"] / nbytes) / (med["convert"] / cbytes)
        print(json.dumps({"case": key, "what": label, "pictures": n, "reformat_ms_median": round(med["reformat"], 4),
                          "reformat_ms_min": round(best["reformat"], 4), "convert_ms_median": round(med["convert"], 4),
                          "convert_ms_min": round(best["convert"], 4), "bytes": n * nbytes, "convert_bytes": n * cbytes,
                          "reformat_TBps": round(n * nbytes / (med["reformat"] * 1e-3) / 1e12, 2), "time_per_byte_to_convert": round(ratio, 3),
                          "time_per_byte_to_convert_min": round((best["reformat"] / nbytes) / (best["convert"] / cbytes), 3),
                          "expected_within": margin, "inside": ratio <= margin}), flush=True)
    eng.close()


def summarize(a):
    """kernel times of a rocprofv3 --kernel-trace --stats run of this tool: each case's reformat dispatches beside the conversion's of
    the same sources, median and minimum, and the time per byte relative to the conversion"""
    paths = sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {a.summarize}")
    rows = sorted(csv.DictReader(open(paths[-1])), key=lambda r: int(r["Start_Timestamp"]))

    def find(kernel):
        return [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows if kernel + "<" in r["Kernel_Name"]]
    per_case = 1 + a.reps * a.rounds                        # the warm-up and the timed calls, in the order of CASES
    rf, cv = find("reformat_kernel")[SETUP_CALLS:], find("convert_yuv_kernel")
    if len(rf) != len(CASES) * per_case or len(cv) != len(CASES) * per_case:
        sys.exit(f"{len(rf)} reformat and {len(cv)} conversion dispatches: not {len(CASES)} cases of 1 + {a.reps} x {a.rounds}; pass the run's "
                 "--pictures (at most 64), --reps and --rounds")
    n = a.pictures
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {n} pictures {W}x{H} per call; per byte: (reformat time / reformat bytes) / (convert time / convert bytes)")
    print(f"# {'case':48s} {'calls':>5s} {'med us':>8s} {'min us':>8s} {'MB/call':>8s} {'TB/s':>5s} | {'convert med us':>14s} {'MB/call':>8s} {'TB/s':>5s} | "
          f"{'per byte, med':>13s} {'min':>6s} {'within':>6s} {'inside':>6s}")
    for i, (key, label, s, d, kw, margin) in enumerate(CASES):
        v, c = sorted(t for _, t in rf[i * per_case:(i + 1) * per_case]), sorted(t for _, t in cv[i * per_case:(i + 1) * per_case])
        m, lo, cm, cmin = v[len(v) // 2], v[0], c[len(c) // 2], c[0]
        nbytes, cbytes = planes(*s) + planes(*d), 2 * planes(*s)
        r, rmin = (m / nbytes) / (cm / cbytes), (lo / nbytes) / (cmin / cbytes)
        print(f"  ({key}) {label:44s} {len(v):5d} {m:8.1f} {lo:8.1f} {n * nbytes / 1e6:8.1f} {n * nbytes / (m * 1e-6) / 1e12:5.2f} | {cm:14.1f} "
              f"{n * cbytes / 1e6:8.1f} {n * cbytes / (cm * 1e-6) / 1e12:5.2f} | {r:13.3f} {rmin:6.3f} {margin:6.2f} {'yes' if r <= margin else 'NO':>6s}")
        print(f"#       kernels: {rf[i * per_case][0]}; {cv[i * per_case][0]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--summarize", metavar="DIR", help="read the rocprofv3 --kernel-trace output under DIR instead of running")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)


if __name__ == "__main__":
    main()
