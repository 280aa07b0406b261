"""Rate of the picture conversion (oh_pics_convert): 32 pictures of 3840x2160 4:2:0, Main 10 and the same pictures at 8 bit, converted
in one call into each of P010 / NV12 (semi-planar, native samples), I420 u8, RGB u8 interleaved, RGB f16 planar and RGB f32 planar
(BT.709, limited range, linear chroma).  Bytes per call, from the shapes: the window's planes read plus the images written.

    python tools/convert_rate.py                        device time per call with events on the engine's stream (no profiler)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o conv -- python tools/convert_rate.py --reps 20
    python tools/convert_rate.py --summarize OUT         kernel times of that run (its *kernel_stats.csv) -> GB/s per format
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 3840, 2160
# (label at 10 bit, label at 8 bit, format, dtype name, the kernel instantiation: (kernel, output sample, layout) as convert.hip names them)
FORMS = [("P010", "NV12", "semiplanar", None, ("yuv", None, 1)),
         ("I420 u8", "I420 u8", "planar", "uint8", ("yuv", 0, 0)),
         ("RGB u8", "RGB u8", "rgb", "uint8", ("rgb", 0, 3)),
         ("RGB f16 planar", "RGB f16 planar", "rgb_planar", "float16", ("rgb", 2, 2)),
         ("RGB f32 planar", "RGB f32 planar", "rgb_planar", "float32", ("rgb", 3, 2))]


def call_bytes(bd, fmt, dtype, n):
    """bytes one call moves: the window's three planes read, the n images written"""
    bps = 2 if bd > 8 else 1
    read = W * H * 3 // 2 * bps
    out_bps = {None: bps, "uint8": 1, "float16": 2, "float32": 4}[dtype]
    written = (W * H * 3 // 2 if fmt in ("planar", "semiplanar") else W * H * 3) * out_bps
    return n * (read + written)


def label(bd, form):
    return f"{form[0] if bd > 8 else form[1]} from {bd} bit"


def run(a):
    import torch

    from openhevc_amd import frame as F
    from openhevc_amd.engine import Engine
    stream = torch.cuda.current_stream()
    eng = Engine(0, stream=stream.cuda_stream)               # on torch's stream: torch events time the engine's launches
    rng = np.random.default_rng(1)
    res = []
    for bd in (10, 8):
        p = F.pic_params(W, H, bit_depth=bd, chroma_format_idc=1)
        base = F.HostPic(p, rng=rng)
        pids = []
        for k in range(a.pictures):
            hp = F.HostPic(p)
            for c in range(3):
                hp.visible(c)[...] = (base.visible(c).astype(np.int64) + 37 * k) & ((1 << bd) - 1)
            pid = eng.pic_alloc(p)
            eng.pic_upload(pid, hp)
            pids.append(pid)
        eng.sync()
        for form in FORMS:
            _, _, fmt, dt, _ = form
            kw = dict(dtype=getattr(torch, dt) if dt else None, matrix=1, full_range=False, chroma="linear")
            out = eng.pics_convert(pids, fmt, **kw)          # warm-up; the same tensor is reused
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                eng.pics_convert(pids, fmt, out=out, **kw)
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            nb = call_bytes(bd, fmt, dt, a.pictures)
            res.append({"form": label(bd, form), "pictures": a.pictures, "bytes": nb, "call_ms": round(ms, 4),
                        "TBps": round(nb / (ms * 1e-3) / 1e12, 2)})
            print(json.dumps(res[-1]), flush=True)
            del out
        for pid in pids:
            eng.pic_free(pid)
    eng.close()


def summarize(a):
    """kernel times of a rocprofv3 --stats run of this tool -> GB/s per format"""
    paths = sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_stats.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_stats.csv under {a.summarize}")
    rows = list(csv.DictReader(open(paths[-1])))
    pat = re.compile(r"convert_(yuv|rgb)_kernel<unsigned (char|short), (\d), (\d)>")
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {a.pictures} pictures {W}x{H} 4:2:0 per call; "
          "bytes = window planes read + images written")
    print(f"# {'form':26s} {'kernel':44s} {'calls':>5s} {'avg us':>9s} {'min us':>9s} {'MB/call':>9s} {'TB/s avg':>8s} {'TB/s min':>8s}")
    for r in rows:
        m = pat.search(r["Name"])
        if not m:
            continue
        kind, ti, o, lay = m.group(1), m.group(2), int(m.group(3)), int(m.group(4))
        bd = 10 if ti == "short" else 8
        for form in FORMS:
            k, fo, fl = form[4]
            if k == kind and fl == lay and (fo is None or fo == o) and not (kind == "yuv" and fo is None and o != (1 if bd > 8 else 0)):
                break
        else:
            continue
        nb = call_bytes(bd, form[2], form[3], a.pictures)
        avg, mn = float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3
        name = f"{kind}<{ti},{o},{lay}>"
        print(f"  {label(bd, form):26s} {name:44s} {int(r['Calls']):5d} {avg:9.1f} {mn:9.1f} {nb / 1e6:9.1f} "
              f"{nb / (avg * 1e-6) / 1e12:8.2f} {nb / (mn * 1e-6) / 1e12:8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summarize", metavar="DIR", help="read the rocprofv3 --stats output under DIR instead of running")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)


if __name__ == "__main__":
    main()
