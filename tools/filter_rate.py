"""Rate of oh_pics_filter beside oh_pics_reformat to the same bit depth and chroma format of the same pictures in the same run — a copy
of the coded planes by existing code: 32 pictures of 3840x2160 4:2:0 per call, at 10 and at 8 bit, the cases
  (c3) (c9) (c15) CONVOLVE with binomial 3 x 3, binomial 9 x 9 and 15 x 15 taps with negative lobes, both classes alike
  (u) UNSHARP with binomial 3 x 3   (m) MEDIAN   (t) TEMPORAL, with prev and next of their own
Every case writes the bytes of 32 coded pictures, as the copy does, so the figure is time per destination byte relative to the copy.
TEMPORAL reads three pictures where the copy reads one: beside its ratio stands the ratio to a copy that read three (its time scaled by
the bytes moved, 4 : 2).  Host wall time per call around `reps` calls and a wait for the engine stream; case and copy alternate, `rounds`
times; the figures are the median and the best round.  The kernels alone come from a profiler run of its own, without counters:

    python tools/filter_rate.py [--pictures 32] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o filter -- python tools/filter_rate.py --reps 10 --rounds 2
    python tools/filter_rate.py --summarize OUT --reps 10 --rounds 2      kernel times of that run (its *kernel_trace.csv) per case;
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
LOBES15 = [-8, -16, -24, -16, 0, 48, 80, 128, 80, 48, 0, -16, -24, -8, -16]


def planes(bd, w=W, h=H):
    """bytes of the coded planes of one 4:2:0 picture"""
    return w * h * 3 // 2 * (2 if bd > 8 else 1)


# (key, label, pictures read per picture written)
SHAPES = [("c3", "convolve 3x3", 1), ("c9", "convolve 9x9", 1), ("c15", "convolve 15x15", 1), ("u", "unsharp 3x3", 1), ("m", "median", 1),
          ("t", "temporal", 3)]
CASES = [(f"{key}/{bd}", f"{label}, {bd} bit", bd, key, reads) for bd in (10, 8) for key, label, reads in SHAPES]
SETUP_COPIES = 3                                            # reformat calls in front of the cases: the 8-bit prev, cur and next


def run(a):
    import torch

    from openhevc_amd import engine as E
    eng = E.Engine(0)
    n = a.pictures
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(15)

    def imported():
        yuv = torch.randint(0, 1024, (n, H * 3 // 2, W), dtype=torch.int16, device=dev, generator=g).view(torch.uint16)
        return eng.pics_import(yuv, "planar", bit_depth=10, chroma_format_idc=1)[0]
    f10 = [imported() for _ in range(3)]                    # prev, cur, next
    sets = {10: f10, 8: [eng.pics_reformat(v, bit_depth=8) for v in f10]}
    eng.sync()
    b3, b9 = E.filter_binomial(3), E.filter_binomial(9)
    how = {"c3": ("convolve", dict(luma=(b3, b3), chroma=(b3, b3))), "c9": ("convolve", dict(luma=(b9, b9), chroma=(b9, b9))),
           "c15": ("convolve", dict(luma=(LOBES15, LOBES15), chroma=(LOBES15, LOBES15))),
           "u": ("unsharp", dict(luma=(b3, b3), chroma=(b3, b3), amount=64, threshold=2)), "m": ("median", dict()),
           "t": ("temporal", dict(threshold=(12, 12)))}
    dst, copies = {}, {}
    for key, label, bd, what, reads in CASES:
        prv, cur, nxt = sets[bd]
        if bd not in dst:
            dst[bd] = eng._alloc_like(eng._pic_params(cur[0]), n)
            copies[bd] = eng._alloc_like(eng._pic_params(cur[0]), n)
        cp, d = copies[bd], dst[bd]
        mode, kw = how[what]

        def case():
            eng.pics_filter(cur, mode, prev=prv, next=nxt, out=d, **kw)

        def copy():
            eng.pics_reformat(cur, out=cp)

        case()                                              # warm-up
        copy()
        eng.sync()

        def timed(fn):
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            eng.sync()
            return (time.perf_counter() - t0) / a.reps * 1e3

        ms = {"case": [], "copy": []}
        for _ in range(a.rounds):
            ms["case"].append(timed(case))
            ms["copy"].append(timed(copy))
        med = {k: statistics.median(v) for k, v in ms.items()}
        best = {k: min(v) for k, v in ms.items()}
        out_bytes = n * planes(bd)
        moved = int(out_bytes * (reads + 1))
        row = {"case": key, "what": label, "pictures": n, "ms_median": round(med["case"], 4), "ms_min": round(best["case"], 4),
               "copy_ms_median": round(med["copy"], 4), "copy_ms_min": round(best["copy"], 4), "dst_bytes": out_bytes, "bytes_moved": moved,
               "TBps_moved": round(moved / (med["case"] * 1e-3) / 1e12, 2),
               "time_per_dst_byte_to_copy": round(med["case"] / med["copy"], 3),
               "time_per_dst_byte_to_copy_min": round(best["case"] / best["copy"], 3)}
        if reads == 3:
            row["to_a_copy_reading_three"] = round(med["case"] / med["copy"] * 2 / (reads + 1), 3)
        print(json.dumps(row), flush=True)
    eng.close()


def summarize(a):
    """kernel times of a rocprofv3 --kernel-trace --stats run of this tool: each case's dispatches beside the copy's of the same
    pictures, median and minimum, and the time per destination byte relative to the copy"""
    paths = sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {a.summarize}")
    rows = sorted(csv.DictReader(open(paths[-1])), key=lambda r: int(r["Start_Timestamp"]))

    def find(kernel):
        return [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows if kernel in r["Kernel_Name"]]
    timed = a.reps * a.rounds
    mine = find("filter_kernel<")
    cp = find("reformat_kernel<")[SETUP_COPIES:]
    want = len(CASES) * (1 + timed)                         # per case one warm-up and the timed calls, of the case and of the copy
    if len(mine) != want or len(cp) != want:
        sys.exit(f"{len(mine)} filter and {len(cp)} copy dispatches, not {want} each: pass the run's --pictures (at most 64), --reps and --rounds")
    n = a.pictures
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {n} pictures {W}x{H} per call; per destination byte: case time / copy time (equal bytes written)")
    print(f"# {'case':28s} {'calls':>5s} {'med us':>8s} {'min us':>8s} {'MB moved':>9s} {'TB/s':>5s} | {'copy med us':>11s} {'TB/s':>5s} | "
          f"{'to copy, med':>12s} {'min':>6s} {'to a copy reading three':>24s}")
    for i, (key, label, bd, what, reads) in enumerate(CASES):
        at = i * (1 + timed) + 1
        v, c = mine[at:at + timed], cp[at:at + timed]
        names = {k for k, _ in v}
        vt, ct = sorted(t for _, t in v), sorted(t for _, t in c)
        m, lo, cm, cmin = vt[len(vt) // 2], vt[0], ct[len(ct) // 2], ct[0]
        moved, cmoved = int(n * planes(bd) * (reads + 1)), n * planes(bd) * 2
        extra = f"{m / cm * 2 / (reads + 1):24.3f}" if reads == 3 else ""
        print(f"  ({key:6s}) {label:19s} {len(vt):5d} {m:8.1f} {lo:8.1f} {moved / 1e6:9.1f} {moved / (m * 1e-6) / 1e12:5.2f} | {cm:11.1f} "
              f"{cmoved / (cm * 1e-6) / 1e12:5.2f} | {m / cm:12.3f} {lo / cmin:6.3f} {extra}")
        print(f"#       kernels: {'; '.join(sorted(names))}")


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
