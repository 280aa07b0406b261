"""Rate of the colour conversion (oh_pics_convert_colour) beside the plain RGB conversion (oh_pics_convert) of the same pictures to the
same format in the same run: 32 pictures of 3840x2160 4:2:0 Main 10, PQ / BT.2020 (matrix 9, limited range, linear chroma), converted
in one call to
    sRGB / BT.709 with the BT.2390 tone curve (1000 -> 100 nits) as u8 RGB interleaved and as f16 planar,
    linear light in BT.709 primaries, no tone curve, as f16 planar.
Each call is one launch (the tables are on the device after the warm-up), so the device time between two events on the engine's
stream around `reps` calls is the kernels' time.  The two conversions alternate, `rounds` times; the figure is the best round, the
spread is printed.  Bytes per call, from the shapes: the window's planes read plus the images written (the 29 KB of tables a
workgroup reads come out of L2 and are not counted).

    python tools/colour_rate.py [--pictures 32] [--reps 10] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BD = 3840, 2160, 10


def forms(E):
    sdr = E.make_colour(16, 9, out="srgb", out_primaries=1, tone="bt2390", norm="maxrgb", src_peak=1000, dst_peak=100)
    lin = E.make_colour(16, 9, out="linear", out_primaries=1, tone="none", white=203)
    return [("PQ/2020 -> sRGB/709 u8 RGB", "rgb", "uint8", sdr), ("PQ/2020 -> sRGB/709 f16 planar", "rgb_planar", "float16", sdr),
            ("PQ/2020 -> linear/709 f16 planar", "rgb_planar", "float16", lin)]


def call_bytes(dtype, n):
    """bytes one call moves: the three planes read, the n RGB images written"""
    return n * (W * H * 3 // 2 * 2 + W * H * 3 * {"uint8": 1, "float16": 2}[dtype])


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
    rng = np.random.default_rng(1)
    p = F.pic_params(W, H, bit_depth=BD, chroma_format_idc=1)
    base = F.HostPic(p, rng=rng)
    pids = []
    for k in range(a.pictures):
        hp = F.HostPic(p)
        for c in range(3):
            hp.visible(c)[...] = (base.visible(c).astype(np.int64) + 37 * k) & ((1 << BD) - 1)
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        pids.append(pid)
    eng.sync()

    def timed(out, fmt, kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            eng.pics_convert(pids, fmt, out=out, **kw)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for label, fmt, dt, col in forms(E):
        kw = dict(dtype=getattr(torch, dt), matrix=9, full_range=False, chroma="linear")
        out = eng.pics_convert(pids, fmt, colour=col, **kw)   # warm-up of both kernels; the same tensor is reused
        eng.pics_convert(pids, fmt, out=out, **kw)
        torch.cuda.synchronize()
        ms = {"colour": [], "plain": []}
        for _ in range(a.rounds):
            ms["colour"].append(timed(out, fmt, dict(kw, colour=col)))
            ms["plain"].append(timed(out, fmt, kw))
        nb = call_bytes(dt, a.pictures)
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps({"form": label, "pictures": a.pictures, "bytes": nb,
                          "colour_ms": round(best["colour"], 4), "colour_ms_worst": round(max(ms["colour"]), 4),
                          "plain_ms": round(best["plain"], 4), "plain_ms_worst": round(max(ms["plain"]), 4),
                          "colour_TBps": round(nb / (best["colour"] * 1e-3) / 1e12, 2), "plain_TBps": round(nb / (best["plain"] * 1e-3) / 1e12, 2),
                          "ratio": round(best["colour"] / best["plain"], 2)}), flush=True)
        del out
    eng.close()


if __name__ == "__main__":
    main()
