"""Rate of the picture composition (oh_pics_compose) beside oh_pics_convert to OH_CONV_PLANAR / OH_CONV_NATIVE of the same pictures in
the same run — the conversion is existing code that reads the three planes and writes the same bytes, in effect a copy: 32 pictures of
3840x2160 4:2:0 Main 10 per call, the cases
  (a) the fill alone                                                bytes: the planes, written
  (b) one opaque whole-picture layer, no alpha                      bytes: the source's planes read, the destination's written
  (c) one whole-picture layer with an alpha plane each, opacity 200 bytes: destination read and written, source, one alpha byte per pixel
  (d) a 480x270 logo with alpha at an odd granule offset            time alone: the bounding box is all the call touches
Host wall time per call around `reps` calls and a wait for the engine stream; composition and conversion alternate, `rounds` times;
the figures are the median and the best round.  The kernels alone come from a profiler run of its own, without counters:

    python tools/compose_rate.py [--pictures 32] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o compose -- python tools/compose_rate.py --reps 10 --rounds 2
    python tools/compose_rate.py --summarize OUT --reps 10 --rounds 2     kernel times of that run (its *kernel_trace.csv) per case;
                                                                          cases (b), (c) and (d) run the same kernel and are told apart
                                                                          by their order, so --reps and --rounds must be the run's
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
LW, LH = 480, 270
LOGO_AT = (1002, 500)                                       # 1002 = 125 granules of 8 samples and 2: no source byte is aligned with its destination
PLANES = W * H * 3 // 2 * 2                                 # bytes of the three planes of one picture
# (key, label, bytes per picture, margin the issue expects (None: time alone), kernel as the profiler names it)
CASES = [("a", "fill alone", PLANES, 1.25, "compose_kernel<unsigned short, true>"),
         ("b", "opaque whole-picture layer", 2 * PLANES, 1.25, "compose_kernel<unsigned short, false>"),
         ("c", "whole-picture layer, alpha, opacity 200", 3 * PLANES + W * H, 1.5, "compose_kernel<unsigned short, false>"),
         ("d", "480x270 logo with alpha at (1002, 500)", None, None, "compose_kernel<unsigned short, false>")]
CONVERT_KERNEL = "convert_yuv_kernel<unsigned short, 1, 0>"
CONVERT_BYTES = 2 * PLANES                                  # the planes read, the image written


def run(a):
    import torch

    from openhevc_amd import frame as F
    from openhevc_amd.engine import Engine, Layer
    eng = Engine(0)
    n = a.pictures
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(11)
    sets = []
    for _ in range(2):                                      # destinations and sources: random pictures made on the device
        yuv = torch.randint(0, 1024, (n, H * 3 // 2, W), dtype=torch.int16, device=dev, generator=g).view(torch.uint16)
        ids, _ = eng.pics_import(yuv, "planar", bit_depth=10, chroma_format_idc=1)
        sets.append(ids)
        del yuv
    dst, src = sets
    lp = F.pic_params(LW, (LH + 7) // 8 * 8, bit_depth=10, chroma_format_idc=1)
    yuv = torch.randint(0, 1024, (1, lp.height * 3 // 2, LW), dtype=torch.int16, device=dev, generator=g).view(torch.uint16)
    logo, _ = eng.pics_import(yuv, "planar", out=[eng.pic_alloc(lp)])
    alpha = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device=dev, generator=g)
    logo_alpha = torch.randint(0, 256, (LH, LW), dtype=torch.uint8, device=dev, generator=g)
    eng.sync()
    calls = {"a": lambda: eng.pics_compose(dst, [], fill=(64, 512, 512)),
             "b": lambda: eng.pics_compose(dst, [Layer(src)]),
             "c": lambda: eng.pics_compose(dst, [Layer(src, opacity=200, alpha=alpha)]),
             "d": lambda: eng.pics_compose(dst, [Layer(logo[0], (0, 0, LW, LH), LOGO_AT, 256, logo_alpha)])}
    img = eng.pics_convert(dst, "planar")                   # warm-up; the tensor is reused

    def convert():
        eng.pics_convert(dst, "planar", out=img)

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        eng.sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    for key, label, nbytes, margin, _ in CASES:
        calls[key]()                                        # warm-up
        eng.sync()
        if key == "b":                                      # an opaque whole-picture layer is a copy
            assert all(c.plane[k].differing == 0 for c in eng.pics_compare(src[:2], dst[:2], ssim=False) for k in range(3))
        ms = {"compose": [], "convert": []}
        for _ in range(a.rounds):
            ms["compose"].append(timed(calls[key]))
            ms["convert"].append(timed(convert))
        med = {k: statistics.median(v) for k, v in ms.items()}
        best = {k: min(v) for k, v in ms.items()}
        out = {"case": key, "what": label, "pictures": n, "compose_ms_median": round(med["compose"], 4), "compose_ms_min": round(best["compose"], 4),
               "convert_ms_median": round(med["convert"], 4), "convert_ms_min": round(best["convert"], 4)}
        if nbytes:
            ratio = (med["compose"] / nbytes) / (med["convert"] / CONVERT_BYTES)
            out.update({"bytes": n * nbytes, "convert_bytes": n * CONVERT_BYTES, "compose_TBps": round(n * nbytes / (med["compose"] * 1e-3) / 1e12, 2),
                        "time_per_byte_to_convert": round(ratio, 3),
                        "time_per_byte_to_convert_min": round((best["compose"] / nbytes) / (best["convert"] / CONVERT_BYTES), 3),
                        "expected_within": margin, "inside": ratio <= margin})
        else:
            out["compose_to_whole_picture_convert"] = round(med["compose"] / med["convert"], 4)
        print(json.dumps(out), flush=True)
    eng.close()


def summarize(a):
    """kernel times of a rocprofv3 --kernel-trace --stats run of this tool: each case's compose dispatches beside the conversion's,
    median and minimum, and the time per byte relative to the conversion"""
    paths = sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {a.summarize}")
    rows = sorted(csv.DictReader(open(paths[-1])), key=lambda r: int(r["Start_Timestamp"]))
    us = {}
    for r in rows:
        us.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)

    def find(kernel):
        for name, v in us.items():
            if kernel + "(" in name:
                return v
        return []
    per_case = 1 + a.reps * a.rounds                        # the warm-up and the timed calls, in the order of CASES
    shared = find(CASES[1][4])
    if len(shared) != 3 * per_case:
        sys.exit(f"{len(shared)} dispatches of {CASES[1][4]}: not 3 cases of 1 + {a.reps} x {a.rounds}; pass the run's --reps and --rounds")
    conv = sorted(find(CONVERT_KERNEL))
    if not conv:
        sys.exit(f"no dispatch of {CONVERT_KERNEL}")
    cm, cmin = conv[len(conv) // 2], conv[0]
    n = a.pictures
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {n} pictures {W}x{H} 4:2:0 Main 10 per call")
    print(f"# conversion to planar native samples: {len(conv)} calls, median {cm:.1f} us, min {cmin:.1f} us, {n * CONVERT_BYTES / 1e6:.1f} MB/call, "
          f"{n * CONVERT_BYTES / (cm * 1e-6) / 1e12:.2f} TB/s")
    print(f"# {'case':44s} {'calls':>5s} {'med us':>8s} {'min us':>8s} {'MB/call':>8s} {'TB/s':>5s} {'per byte, med':>13s} {'min':>6s} {'within':>6s} {'inside':>6s}")
    for i, (key, label, nbytes, margin, kernel) in enumerate(CASES):
        v = sorted(find(kernel) if key == "a" else shared[(i - 1) * per_case:i * per_case])
        if not v:
            continue
        m, lo = v[len(v) // 2], v[0]
        if nbytes:
            r, rmin = (m / nbytes) / (cm / CONVERT_BYTES), (lo / nbytes) / (cmin / CONVERT_BYTES)
            print(f"  ({key}) {label:40s} {len(v):5d} {m:8.1f} {lo:8.1f} {n * nbytes / 1e6:8.1f} {n * nbytes / (m * 1e-6) / 1e12:5.2f} {r:13.3f} {rmin:6.3f} "
                  f"{margin:6.2f} {'yes' if r <= margin else 'NO':>6s}")
        else:
            print(f"  ({key}) {label:40s} {len(v):5d} {m:8.1f} {lo:8.1f} {'-':>8s} {'-':>5s} {'-':>13s} {'-':>6s} {'-':>6s} {'-':>6s}   "
                  f"{m / cm:.4f} of the conversion of the whole pictures")


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
