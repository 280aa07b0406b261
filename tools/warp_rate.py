"""Rate of oh_pics_warp on 32 pictures of 3840x2160 4:2:0 per call, at 10 and at 8 bit, beside yardsticks of existing code on the same
pictures in the same run: oh_pics_reformat to the same depth and format (a copy of the coded planes: time per destination byte relative
to the copy), oh_pics_orient where the map is a quarter turn, and oh_pics_resize where it is a scale by 3/4.

  identity, rot30 (30 degrees about the centre), keystone (perspective)   nearest / bilinear / bicubic, into 3840x2160
  quarter    a quarter turn anticlockwise into 2160x3840, beside oh_pics_orient
  scale34    a scale by 3/4 into 2880x1624 (point-sampled: no anti-aliasing), beside oh_pics_resize
  down8      the 8 : 1 map of the whole picture into 480x272, whose tiles gather from global memory (oh_warp_paths says so in the output)

Host wall time per call around `reps` calls and a wait for the engine stream; case and yardstick alternate, `rounds` times; the figures
are the median and the range of the rounds.

    python tools/warp_rate.py [--pictures 32] [--reps 3] [--rounds 5]
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
ONE, ONE30 = 1 << 16, 1 << 30


def planes(bd, w, h):
    """bytes of the coded planes of one 4:2:0 picture"""
    return w * h * 3 // 2 * (2 if bd > 8 else 1)


def run(a):
    import torch

    from openhevc_amd import engine as E
    eng = E.Engine(0)
    n = a.pictures
    g = torch.Generator(device="cuda:0").manual_seed(20)
    yuv = torch.randint(0, 1024, (n, H * 3 // 2, W), dtype=torch.int32, device="cuda:0", generator=g)
    p10 = eng.pics_import(yuv.to(torch.int16).view(torch.uint16), "planar", bit_depth=10, chroma_format_idc=1)[0]
    sets = {10: p10, 8: eng.pics_reformat(p10, bit_depth=8)}
    eng.sync()
    del yuv

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        eng.sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    def beside(case, yards):
        case()
        for y in yards.values():
            y()
        eng.sync()
        ms = {k: [] for k in ["case"] + list(yards)}
        for _ in range(a.rounds):
            ms["case"].append(timed(case))
            for k, y in yards.items():
                ms[k].append(timed(y))
        return ms

    def stats(v):
        return round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)

    centre = ((W - 1) << 15, (H - 1) << 15)
    k6 = -(ONE30 // 4) // (W - 1)                               # the denominator falls to 3/4 across the width
    maps = {"identity": (list(E.warp_identity().m), 0, (W, H)),
            "rot30": (list(E.warp_rotation(5461, centre, centre).m), 0, (W, H)),
            "keystone": ([ONE, 0, 0, 0, ONE, 0, k6, 0, ONE30], 1, (W, H)),
            "quarter": (list(E.warp_from_sei(0, 0, 1 << 14, W, H)[0].m), 0, (H, W)),
            "scale34": ([ONE * 4 // 3, 0, ONE // 6, 0, ONE * 4 // 3, ONE // 6, 0, 0, ONE30], 0, (2880, 1624)),
            "down8": ([8 * ONE, 0, 7 << 15, 0, 8 * ONE, 7 << 15, 0, 0, ONE30], 0, (480, 272))}
    for bd in (10, 8):
        src = sets[bd]
        sp = eng._pic_params(src[0])
        cp = eng._alloc_like(sp, n)
        for name, (m, mode, size) in maps.items():
            dst = eng._alloc_like(eng._sized(sp, *size), n)
            dp = eng._pic_params(dst[0])
            yards = {"copy": lambda: eng.pics_reformat(src, out=cp)}
            if name == "quarter":
                yards["orient"] = lambda: eng.pics_orient(src, "rot270", out=dst)
            if name == "scale34":
                yards["resize"] = lambda: eng.pics_resize(src, size, filter="bilinear", out=dst)
            for filt in ("nearest", "bilinear", "bicubic"):
                if name not in ("identity", "rot30", "keystone") and filt != "bilinear":
                    continue
                w = E.warp_identity()
                w.mode, w.filter, w.width, w.height = mode, E.WARP_FILTERS[filt], size[0], size[1]
                for k, v in enumerate(m):
                    w.m[k] = v
                staged, gathered = E.warp_paths(w, bd, 1, dp.width, dp.height)
                ms = beside(lambda: eng.pics_warp(src, m, size, mode=mode, filter=filt, out=dst), yards)
                med, lo, hi = stats(ms["case"])
                cmed, clo, chi = stats(ms["copy"])
                per_byte = (med / planes(bd, dp.width, dp.height)) / (cmed / planes(bd, W, H))
                row = {"map": name, "filter": filt, "bits": bd, "pictures": n, "image": list(size), "tiles_staged": staged, "tiles_gathered": gathered,
                       "ms_median": med, "ms_min": lo, "ms_max": hi, "copy_ms_median": cmed, "copy_ms_min": clo, "copy_ms_max": chi,
                       "dst_bytes": n * planes(bd, dp.width, dp.height), "time_per_dst_byte_to_copy": round(per_byte, 2)}
                for k in yards:
                    if k != "copy":
                        ymed, ylo, yhi = stats(ms[k])
                        row.update({f"{k}_ms_median": ymed, f"{k}_ms_min": ylo, f"{k}_ms_max": yhi, f"to_{k}": round(med / ymed, 2)})
                print(json.dumps(row), flush=True)
            for pid in dst:
                eng.pic_free(pid)
        for pid in cp:
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
