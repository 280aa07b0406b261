"""Rate of the picture resizing (oh_pics_resize): 32 pictures of 4:2:0, Main 10 and the same pictures at 8 bit, resized in one call
3840x2160 -> 224x224, 3840x2160 -> 1920x1080 and 1920x1080 -> 3840x2160, with both filters.  Bytes per call, from the shapes: the
window's planes read plus the image planes written (the int16 intermediate is the engine's business and is not counted).  Beside
each line the installed torch's own resampler: the same planes, already on the device as float16 tensors (their conversion is not
counted), through torch.nn.functional.interpolate(..., antialias=True) — one call for the luma planes, one for the chroma planes.

    python tools/resize_rate.py                         device time per call with events on the engine's stream (no profiler)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o resize -- python tools/resize_rate.py --reps 20 --no-torch
    python tools/resize_rate.py --summarize OUT --reps 20   kernel times of that run (its *kernel_trace.csv), per line and pass
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (source size, image size); every image size here is a multiple of 8, so no call launches the padding kernel: two launches per call
GEOMS = [((3840, 2160), (224, 224)), ((3840, 2160), (1920, 1080)), ((1920, 1080), (3840, 2160))]
FILTERS = ("bilinear", "bicubic")
DEPTHS = (10, 8)


def lines():
    """the table's lines in the order the tool runs them"""
    return [(bd, src, dst, filt) for bd in DEPTHS for src, dst in GEOMS for filt in FILTERS]


def call_bytes(bd, src, dst, n):
    bps = 2 if bd > 8 else 1
    return n * (src[0] * src[1] + dst[0] * dst[1]) * 3 // 2 * bps


def label(bd, src, dst, filt):
    return f"{src[0]}x{src[1]} -> {dst[0]}x{dst[1]} {filt} {bd} bit"


def timed(torch, stream, reps, fn):
    fn()                                                      # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run(a):
    import torch
    import torch.nn.functional as TF

    from openhevc_amd import frame as F
    from openhevc_amd.engine import Engine
    stream = torch.cuda.current_stream()
    eng = Engine(0, stream=stream.cuda_stream)               # on torch's stream: torch events time the engine's launches
    rng = np.random.default_rng(1)
    for bd in DEPTHS:
        for src, dst in GEOMS:
            p = F.pic_params(src[0], src[1], bit_depth=bd, chroma_format_idc=1)
            base = F.HostPic(p, rng=rng)
            pids, luma, chroma = [], [], []
            for k in range(a.pictures):
                hp = F.HostPic(p)
                for c in range(3):
                    hp.visible(c)[...] = (base.visible(c).astype(np.int64) + 37 * k) & ((1 << bd) - 1)
                pid = eng.pic_alloc(p)
                eng.pic_upload(pid, hp)
                pids.append(pid)
                if not a.no_torch:
                    luma.append(torch.from_numpy(hp.visible(0).astype(np.float16)))
                    chroma += [torch.from_numpy(hp.visible(c).astype(np.float16)) for c in (1, 2)]
            eng.sync()
            if not a.no_torch:
                t_luma = torch.stack(luma)[:, None].cuda()    # N x 1 x H x W, float16
                t_chroma = torch.stack(chroma)[:, None].cuda()
            out = None
            for filt in FILTERS:
                def ours():
                    nonlocal out
                    out, _ = eng.pics_resize(pids, dst, filter=filt, out=out)
                ms = timed(torch, stream, a.reps, ours)
                nb = call_bytes(bd, src, dst, a.pictures)
                res = {"line": label(bd, src, dst, filt), "pictures": a.pictures, "bytes": nb, "call_ms": round(ms, 4),
                       "TBps": round(nb / (ms * 1e-3) / 1e12, 2)}
                if not a.no_torch:
                    def theirs():
                        TF.interpolate(t_luma, size=(dst[1], dst[0]), mode=filt, antialias=True, align_corners=False)
                        TF.interpolate(t_chroma, size=(dst[1] // 2, dst[0] // 2), mode=filt, antialias=True, align_corners=False)
                    try:
                        res["torch_f16_ms"] = round(timed(torch, stream, max(1, a.reps // 2), theirs), 4)
                        res["torch_over_engine"] = round(res["torch_f16_ms"] / ms, 2)
                    except RuntimeError as e:                 # said as it is: the installed torch cannot do this line
                        res["torch_f16_ms"] = None
                        res["torch_error"] = str(e).splitlines()[0][:160]
                print(json.dumps(res), flush=True)
            for pid in pids + (out or []):
                eng.pic_free(pid)
            if not a.no_torch:
                del t_luma, t_chroma
                torch.cuda.empty_cache()
    eng.close()


def summarize(a):
    """kernel times of a rocprofv3 --kernel-trace run of this tool (--no-torch, the same --reps and --pictures): the resize kernels in
    start order are (1 warm-up + reps) calls of (horizontal, vertical) per line"""
    paths = sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {a.summarize}")
    k = []
    for r in csv.DictReader(open(paths[-1])):
        if "resize_" in r["Kernel_Name"]:
            k.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    k.sort()
    per = 2 * (a.reps + 1)
    if len(k) != per * len(lines()):
        sys.exit(f"{len(k)} resize launches in the trace, expected {per * len(lines())}: not a run with --reps {a.reps} --no-torch")
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {a.pictures} pictures 4:2:0 per call, {a.reps} calls per line after one warm-up; "
          "bytes = window planes read + image planes written")
    print(f"# {'line':44s} {'h avg us':>9s} {'v avg us':>9s} {'sum avg':>9s} {'sum min':>9s} {'MB/call':>9s} {'TB/s avg':>8s}")
    for i, (bd, src, dst, filt) in enumerate(lines()):
        calls = k[i * per + 2:(i + 1) * per]                  # without the warm-up
        assert all("resize_h" in c[2] for c in calls[0::2]) and all("resize_v" in c[2] for c in calls[1::2])
        h = [(e - s) / 1e3 for s, e, _ in calls[0::2]]
        v = [(e - s) / 1e3 for s, e, _ in calls[1::2]]
        tot = [x + y for x, y in zip(h, v)]
        nb = call_bytes(bd, src, dst, a.pictures)
        avg = sum(tot) / len(tot)
        print(f"  {label(bd, src, dst, filt):44s} {sum(h) / len(h):9.1f} {sum(v) / len(v):9.1f} {avg:9.1f} {min(tot):9.1f} {nb / 1e6:9.1f} "
              f"{nb / (avg * 1e-6) / 1e12:8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true", help="leave torch's interpolate out (the profiler run: only the engine's kernels)")
    ap.add_argument("--summarize", metavar="DIR", help="read the rocprofv3 --kernel-trace output under DIR instead of running")
    a = ap.parse_args()
    summarize(a) if a.summarize else run(a)


if __name__ == "__main__":
    main()
