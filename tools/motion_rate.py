"""Rate of oh_pics_motion and oh_pics_motion_compensate on 32 pairs of 3840x2160 4:2:0 pictures per call, at 10 and at 8 bit, on noise
and on smooth content (cur is ref panned by a few samples, so there is a displacement to find), each beside a yardstick of existing code
on the same pictures in the same run:

  search        block 8 / 16, range 0 / 8 / 16 / 32, subpel 0 / 2, beside oh_pics_compare without SSIM of the same pairs.  At range 0 and
                subpel 0 the search reads the same two luma planes once and forms the same absolute differences (the comparison reads
                chroma too: 1.5 times the bytes), so that ratio judges the staging; the larger ranges are reported as candidate SADs
                per second, (2 rx + 1)(2 ry + 1) + 9 per sub-sample stage candidates per block.
  compensation  block 8 / 16, a zero field and a random quarter-sample field, beside oh_pics_reformat to the same depth and format, a
                copy of the coded planes: time per destination byte relative to the copy.

Host wall time per call around `reps` calls and a wait for the engine stream (the search waits itself and brings its vectors to the
host: that is part of the call); case and yardstick alternate, `rounds` times; the figures are the median and the range of the rounds.

    python tools/motion_rate.py [--pictures 32] [--reps 3] [--rounds 5] [--only search|compensate]
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
RANGES = (0, 8, 16, 32)


def planes(bd, w=W, h=H):
    """bytes of the coded planes of one 4:2:0 picture"""
    return w * h * 3 // 2 * (2 if bd > 8 else 1)


def run(a):
    import numpy as np
    import torch

    from openhevc_amd import engine as E
    eng = E.Engine(0)
    n = a.pictures
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(19)

    def imported(yuv):
        return eng.pics_import(yuv.to(torch.int16).view(torch.uint16), "planar", bit_depth=10, chroma_format_idc=1)[0]

    def content(kind):
        if kind == "noise":
            ref = torch.randint(0, 1024, (n, H * 3 // 2, W), dtype=torch.int32, device=dev, generator=g)
        else:                                               # low-pass noise: a coarse grid enlarged bilinearly
            coarse = torch.rand((n, 1, H * 3 // 2 // 24 + 2, W // 24 + 2), device=dev, generator=g)
            ref = (torch.nn.functional.interpolate(coarse, size=(H * 3 // 2, W), mode="bilinear", align_corners=False)[:, 0] * 1023).to(torch.int32)
        cur = torch.roll(ref, (3, -5), dims=(1, 2))        # the luma rows above the chroma rows: panned alike, which is all that counts here
        return imported(cur), imported(ref)

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        eng.sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    def beside(case, yard):
        case()
        yard()
        eng.sync()
        ms = {"case": [], "yard": []}
        for _ in range(a.rounds):
            ms["case"].append(timed(case))
            ms["yard"].append(timed(yard))
        return ms

    def stats(v):
        return round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)

    for kind in ("noise", "smooth"):
        c10, r10 = content(kind)
        sets = {10: (c10, r10), 8: (eng.pics_reformat(c10, bit_depth=8), eng.pics_reformat(r10, bit_depth=8))}
        eng.sync()
        for bd in (10, 8):
            cur, ref = sets[bd]
            if a.only in (None, "search"):
                for block in (8, 16):
                    bw, bh = E.motion_blocks(W, H, block)
                    for r in RANGES:
                        for subpel in (0, 2):
                            if kind == "smooth" and r not in (0, 8):
                                continue
                            ms = beside(lambda: eng.pics_motion(cur, ref, block=block, range=(r, r), subpel=subpel),
                                        lambda: eng.pics_compare(cur, ref, ssim=False))
                            med, lo, hi = stats(ms["case"])
                            ymed, ylo, yhi = stats(ms["yard"])
                            cands = (2 * r + 1) ** 2 + 9 * subpel
                            print(json.dumps({"call": "search", "content": kind, "bits": bd, "block": block, "range": r, "subpel": subpel, "pairs": n,
                                              "ms_per_pair_median": round(med / n, 4), "ms_per_pair_min": round(lo / n, 4),
                                              "ms_per_pair_max": round(hi / n, 4), "compare_ms_per_pair_median": round(ymed / n, 4),
                                              "compare_ms_per_pair_min": round(ylo / n, 4), "compare_ms_per_pair_max": round(yhi / n, 4),
                                              "to_compare": round(med / ymed, 2), "candidates_per_block": cands,
                                              "G_candidate_SADs_per_s": round(cands * bw * bh * n / (med * 1e-3) / 1e9, 2),
                                              "G_sample_differences_per_s": round(cands * W * H * n / (med * 1e-3) / 1e9, 1)}), flush=True)
            if a.only in (None, "compensate") and kind == "noise":
                p = eng._pic_params(ref[0])
                dst, cp = eng._alloc_like(p, n), eng._alloc_like(p, n)
                for block in (8, 16):
                    bw, bh = E.motion_blocks(W, H, block)
                    rng = np.random.default_rng(block)
                    fields = {"zero": np.zeros((n, bh, bw, 2), np.int16), "quarter": rng.integers(-64, 65, (n, bh, bw, 2)).astype(np.int16)}
                    for name, f in fields.items():
                        f = E.motion_field(f)
                        ms = beside(lambda: eng.pics_motion_compensate(ref, f, block=block, out=dst), lambda: eng.pics_reformat(ref, out=cp))
                        med, lo, hi = stats(ms["case"])
                        ymed, ylo, yhi = stats(ms["yard"])
                        print(json.dumps({"call": "compensate", "bits": bd, "block": block, "field": name, "pictures": n, "ms_median": med, "ms_min": lo,
                                          "ms_max": hi, "copy_ms_median": ymed, "copy_ms_min": ylo, "copy_ms_max": yhi, "dst_bytes": n * planes(bd),
                                          "time_per_dst_byte_to_copy": round(med / ymed, 2), "time_per_dst_byte_to_copy_min": round(lo / ylo, 2)}),
                              flush=True)
                for pid in dst + cp:
                    eng.pic_free(pid)
        for pid in [v for pair in sets.values() for ids in pair for v in ids]:
            eng.pic_free(pid)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("search", "compensate"))
    run(ap.parse_args())


if __name__ == "__main__":
    main()
