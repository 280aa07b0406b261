"""Rate of the field services (oh_pics_weave, oh_pics_separate, oh_pics_deinterlace) beside oh_pics_reformat to the same bit depth and
chroma format of the same pictures in the same run — a copy of the coded planes by existing code: 32 pictures of 3840x2160 4:2:0 per
call, at 10 and at 8 bit, the cases
  (w) weave of 32 + 32 fields of 3840x1080 into 32 frames     (s) separate of 32 frames into 32 + 32 fields
  (0) bob   (1) blend   (2) lowpass5   (3) adaptive, with prev and next of their own
Every case writes the bytes of 32 coded pictures, as the copy does, so the figure is time per destination byte relative to the copy.
ADAPTIVE reads three pictures where the copy reads one: beside its ratio stands the ratio to a copy that read three (its time scaled by
the bytes moved, 4 : 2).  Host wall time per call around `reps` calls and a wait for the engine stream; case and copy alternate, `rounds`
times; the figures are the median and the best round.  The kernels alone come from a profiler run of its own, without counters:

    python tools/deinterlace_rate.py [--pictures 32] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o deint -- python tools/deinterlace_rate.py --reps 10 --rounds 2
    python tools/deinterlace_rate.py --summarize OUT --reps 10 --rounds 2     kernel times of that run (its *kernel_trace.csv) per case;
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


def planes(bd, w=W, h=H):
    """bytes of the coded planes of one 4:2:0 picture"""
    return w * h * 3 // 2 * (2 if bd > 8 else 1)


# (key, label, pictures read per picture written: BOB reads the kept rows only)
SHAPES = [("w", "weave", 1), ("s", "separate", 1), ("0", "bob", 0.5), ("1", "blend", 1), ("2", "lowpass5", 1), ("3", "adaptive", 3)]
CASES = [(f"{key}/{bd}", f"{label}, {bd} bit", bd, key, reads) for bd in (10, 8) for key, label, reads in SHAPES]
SETUP_COPIES = 5                                            # reformat calls in front of the cases: the 8-bit frames and fields


def run(a):
    import torch

    from openhevc_amd.engine import Engine
    eng = Engine(0)
    n = a.pictures
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(14)

    def imported(h):
        yuv = torch.randint(0, 1024, (n, h * 3 // 2, W), dtype=torch.int16, device=dev, generator=g).view(torch.uint16)
        return eng.pics_import(yuv, "planar", bit_depth=10, chroma_format_idc=1)[0]
    f10 = [imported(H) for _ in range(3)]                   # prev, cur, next
    t10, b10 = imported(H // 2), imported(H // 2)
    sets = {10: (f10, t10, b10),
            8: ([eng.pics_reformat(v, bit_depth=8) for v in f10], eng.pics_reformat(t10, bit_depth=8), eng.pics_reformat(b10, bit_depth=8))}
    eng.sync()
    dst, fld, copies = {}, {}, {}
    for key, label, bd, what, reads in CASES:
        (prv, cur, nxt), top, bot = sets[bd]
        if bd not in copies:
            copies[bd] = eng.pics_reformat(cur)                                 # warm-up, allocates
            dst[bd] = eng.pics_reformat(cur)
            fld[bd] = (eng.pics_reformat(top), eng.pics_reformat(bot))
        else:
            eng.pics_reformat(cur, out=copies[bd])
        cp, d, (ft, fb) = copies[bd], dst[bd], fld[bd]

        def case():
            if what == "w":
                eng.pics_weave(top, bot, out=d)
            elif what == "s":
                eng.pics_separate(cur, out=(ft, fb))
            else:
                eng.pics_deinterlace(cur, int(what), prev=prv, next=nxt, out=d)

        def copy():
            eng.pics_reformat(cur, out=cp)

        case()                                              # warm-up
        eng.sync()
        if what == "s":                                     # the fields woven again are the frames
            back = eng.pics_weave(ft[:2], fb[:2])
            assert all(c.plane[k].differing == 0 for c in eng.pics_compare(cur[:2], back, ssim=False) for k in range(3))
            for pid in back:
                eng.pic_free(pid)

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

    def find(*kernels):
        return [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows
                if any(k in r["Kernel_Name"] for k in kernels)]
    timed = a.reps * a.rounds
    mine = find("deint_kernel<", "fields_kernel<")
    cp = find("reformat_kernel<")[SETUP_COPIES:]
    # per bit depth: four reformat warm-ups in front of the first case, one in front of each later one; per case one warm-up of its own,
    # the separate case one weave more (its check)
    want_mine = len(CASES) * (1 + timed) + 2
    want_cp = len(CASES) * timed + 2 * 4 + (len(CASES) - 2)
    if len(mine) != want_mine or len(cp) != want_cp:
        sys.exit(f"{len(mine)} field and {len(cp)} copy dispatches, not {want_mine} and {want_cp}: pass the run's --pictures (at most 64), "
                 "--reps and --rounds")
    n = a.pictures
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {n} pictures {W}x{H} per call; per destination byte: case time / copy time (equal bytes written)")
    print(f"# {'case':28s} {'calls':>5s} {'med us':>8s} {'min us':>8s} {'MB moved':>9s} {'TB/s':>5s} | {'copy med us':>11s} {'TB/s':>5s} | "
          f"{'to copy, med':>12s} {'min':>6s} {'to a copy reading three':>24s}")
    am = ac = 0
    for i, (key, label, bd, what, reads) in enumerate(CASES):
        first = what == "w"
        ac += 4 if first else 1                             # the warm-ups of the copy
        am += 1                                             # the warm-up of the case
        if what == "s":
            am += 1                                         # the check's weave
        v, c = mine[am:am + timed], cp[ac:ac + timed]
        am += timed
        ac += timed
        names = {k for k, _ in v}
        vt, ct = sorted(t for _, t in v), sorted(t for _, t in c)
        m, lo, cm, cmin = vt[len(vt) // 2], vt[0], ct[len(ct) // 2], ct[0]
        moved, cmoved = int(n * planes(bd) * (reads + 1)), n * planes(bd) * 2
        extra = f"{m / cm * 2 / (reads + 1):24.3f}" if reads == 3 else ""
        print(f"  ({key:4s}) {label:21s} {len(vt):5d} {m:8.1f} {lo:8.1f} {moved / 1e6:9.1f} {moved / (m * 1e-6) / 1e12:5.2f} | {cm:11.1f} "
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
