"""Rate of oh_pics_lut and oh_pics_histogram beside existing code over the same pictures in the same run: 32 pictures of 3840x2160
4:2:0 per call, at 10 and at 8 bit, on three contents — uniform noise, a flat picture, and a smooth one (noise of 480x270 enlarged
bicubically by oh_pics_resize: long runs of near-equal values).  The cases
  (l7) oh_pics_lut, all three planes through the inverting table     (l1) luma only, chroma copied
       beside oh_pics_reformat to the same depth and format: a copy of the coded planes.  Both write the bytes of 32 coded pictures, so
       the figure is time per destination byte relative to the copy;
  (h)  oh_pics_histogram beside the checksum pass oh_pics_hash(.., 2): both read every byte of the pictures once and end with a wait
       for the engine stream, so the figure is time per byte read relative to the checksum.
Host wall time per call around `reps` calls and a wait for the engine stream; case and yardstick alternate, `rounds` times; the figures
are the median and the best round, and the spread of the rounds stands beside them.  The kernels alone come from a profiler run of its
own, without counters:

    python tools/levels_rate.py [--pictures 32] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o levels -- python tools/levels_rate.py --reps 10 --rounds 2
    python tools/levels_rate.py --summarize OUT --reps 10 --rounds 2      kernel times of that run (its *kernel_trace.csv) per case;
                                                                          the cases are told apart by their order, so --reps and
                                                                          --rounds must be the run's
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
SW, SH, SPAD = 480, 272, 2                                  # the small noise of the smooth content: 480 x 270 of a 480 x 272 picture
CONTENTS = ("noise", "flat", "smooth")
SHAPES = [("l7", "lut, all planes", "lut"), ("l1", "lut, luma only", "lut"), ("h", "histogram", "hist")]
CASES = [(f"{key}/{bd}/{content}", f"{label}, {bd} bit, {content}", bd, content, key, kind)
         for bd in (10, 8) for content in CONTENTS for key, label, kind in SHAPES]
SETUP_COPIES = len(CONTENTS)                                # reformat calls in front of the cases: the 8-bit pictures of each content


def planes(bd, w=W, h=H):
    """bytes of the coded planes of one 4:2:0 picture"""
    return w * h * 3 // 2 * (2 if bd > 8 else 1)


def run(a):
    import torch

    from openhevc_amd import engine as E
    eng = E.Engine(0)
    n = a.pictures
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(18)

    def imported(yuv):
        return eng.pics_import(yuv, "planar", bit_depth=10, chroma_format_idc=1)[0]

    def noise(w, h):
        return torch.randint(0, 1024, (n, h * 3 // 2, w), dtype=torch.int16, device=dev, generator=g).view(torch.uint16)
    sets = {(10, "noise"): imported(noise(W, H)),
            (10, "flat"): imported(torch.full((n, H * 3 // 2, W), 517, dtype=torch.int16, device=dev).view(torch.uint16)),
            (10, "smooth"): eng.pics_resize(imported(noise(SW, SH)), (W, H), window=(0, 0, 0, SPAD), filter="bicubic")[0]}
    for content in CONTENTS:
        sets[(8, content)] = eng.pics_reformat(sets[(10, content)], bit_depth=8)
    eng.sync()
    dst, copies = {}, {}
    for key, label, bd, content, what, kind in CASES:
        cur = sets[(bd, content)]
        if bd not in dst:
            dst[bd] = eng._alloc_like(eng._pic_params(cur[0]), n)
            copies[bd] = eng._alloc_like(eng._pic_params(cur[0]), n)
        cp, d = copies[bd], dst[bd]
        invert = E.lut_linear(bd, bd, -65536, 0, (1 << bd) - 1)
        if kind == "lut":
            tabs = [invert] * 3 if what == "l7" else [invert, None, None]

            def case():
                eng.pics_lut(cur, tabs, out=d)

            def yard():
                eng.pics_reformat(cur, out=cp)
        else:
            def case():
                eng.pics_histogram(cur)

            def yard():
                eng.pics_hash(cur, 2)

        case()                                              # warm-up
        yard()
        eng.sync()

        def timed(fn):
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            eng.sync()
            return (time.perf_counter() - t0) / a.reps * 1e3

        ms = {"case": [], "yard": []}
        for _ in range(a.rounds):
            ms["case"].append(timed(case))
            ms["yard"].append(timed(yard))
        med = {k: statistics.median(v) for k, v in ms.items()}
        best = {k: min(v) for k, v in ms.items()}
        nbytes = n * planes(bd)                             # written by the lut and the copy; read by the histogram and the checksum
        moved = nbytes * (2 if kind == "lut" else 1)
        row = {"case": key, "what": label, "pictures": n, "ms_median": round(med["case"], 4), "ms_min": round(best["case"], 4),
               "ms_max": round(max(ms["case"]), 4), "yard": "reformat copy" if kind == "lut" else "checksum",
               "yard_ms_median": round(med["yard"], 4), "yard_ms_min": round(best["yard"], 4), "yard_ms_max": round(max(ms["yard"]), 4),
               "bytes": nbytes, "TBps_moved": round(moved / (med["case"] * 1e-3) / 1e12, 2),
               "time_per_byte_to_yard": round(med["case"] / med["yard"], 3), "time_per_byte_to_yard_min": round(best["case"] / best["yard"], 3),
               "spread": round((max(ms["case"]) - best["case"]) / med["case"], 3)}
        print(json.dumps(row), flush=True)
    eng.close()


def summarize(a):
    """kernel times of a rocprofv3 --kernel-trace --stats run of this tool: each case's dispatches beside its yardstick's over the same
    pictures, median and minimum, and the time per byte relative to the yardstick (the checksum: its two kernels of a call added)"""
    paths = sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {a.summarize}")
    rows = sorted(csv.DictReader(open(paths[-1])), key=lambda r: int(r["Start_Timestamp"]))

    def find(kernel):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
    timed = a.reps * a.rounds
    per = 1 + timed                                         # per case one warm-up and the timed calls, of the case and of the yardstick
    n_lut, n_hist = sum(c[5] == "lut" for c in CASES), sum(c[5] == "hist" for c in CASES)
    lut, hist = find("lut_kernel<"), find("histogram_kernel<")
    cp = find("reformat_kernel<")[SETUP_COPIES:]
    part, comb = find("checksum_kernel"), find("hash_combine_kernel")
    if len(lut) != n_lut * per or len(cp) != n_lut * per or len(hist) != n_hist * per or len(part) != n_hist * per or len(comb) != n_hist * per:
        sys.exit(f"{len(lut)} lut, {len(cp)} copy, {len(hist)} histogram, {len(part)} + {len(comb)} checksum dispatches, not {n_lut * per} and "
                 f"{n_hist * per}: pass the run's --pictures (at most 64), --reps and --rounds")
    n = a.pictures
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {n} pictures {W}x{H} per call; per byte: case time / yardstick time")
    print(f"# {'case':50s} {'calls':>5s} {'med us':>8s} {'min us':>8s} {'max us':>8s} {'TB/s':>5s} | {'yard med us':>11s} {'min us':>8s} | {'to yard, med':>12s} {'min':>6s}")
    at = {"lut": 0, "hist": 0}
    for key, label, bd, content, what, kind in CASES:
        i = at[kind] * per + 1
        at[kind] += 1
        if kind == "lut":
            v, y = lut[i:i + timed], cp[i:i + timed]
        else:
            v, y = hist[i:i + timed], [p + c for p, c in zip(part[i:i + timed], comb[i:i + timed])]
        v, y = sorted(v), sorted(y)
        m, lo, ym, ylo = v[len(v) // 2], v[0], y[len(y) // 2], y[0]
        moved = n * planes(bd) * (2 if kind == "lut" else 1)
        print(f"  ({key:14s}) {label:34s} {len(v):5d} {m:8.1f} {lo:8.1f} {v[-1]:8.1f} {moved / (m * 1e-6) / 1e12:5.2f} | {ym:11.1f} {ylo:8.1f} | "
              f"{m / ym:12.3f} {lo / ylo:6.3f}")


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
