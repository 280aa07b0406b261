"""Rate of the picture orientation (oh_pics_orient) beside oh_pics_reformat to the same bit depth and chroma format of the same source
pictures in the same run — a copy of the coded planes by existing code that moves the same bytes: 32 pictures of 3840x2160 4:2:0 per
call, at 10 and at 8 bit, the cases
  (1) hflip   (2) vflip   (3) half turn             the row kernel
  (4) transpose   (5) quarter turn clockwise   (6) quarter turn anticlockwise      the tiled kernel, into 2160x3840 pictures
  (0w) identity with the window (2, 6, 2, 6): a crop to 3832x2152 whose source and destination granules are unaligned to each other
bytes of a call: the window's planes read and the destination's coded planes written; of the copy: the coded planes, read and written.
Host wall time per call around `reps` calls and a wait for the engine stream; orientation and copy alternate, `rounds` times; the
figures are the median and the best round.  The kernels alone come from a profiler run of its own, without counters:

    python tools/orient_rate.py [--pictures 32] [--reps 10] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o orient -- python tools/orient_rate.py --reps 10 --rounds 2
    python tools/orient_rate.py --summarize OUT --reps 10 --rounds 2      kernel times of that run (its *kernel_trace.csv) per case; the
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
CROP = (2, 6, 2, 6)
WHOLE = (0, 0, 0, 0)


def planes(bd, w=W, h=H):
    """bytes of the coded planes of one 4:2:0 picture"""
    return w * h * 3 // 2 * (2 if bd > 8 else 1)


# (key, label, orientation, window)
SHAPES = [("1", "hflip", 1, WHOLE), ("2", "vflip", 2, WHOLE), ("3", "half turn", 3, WHOLE), ("4", "transpose", 4, WHOLE),
          ("5", "quarter turn clockwise", 5, WHOLE), ("6", "quarter turn anticlockwise", 6, WHOLE), ("0w", "identity, window (2, 6, 2, 6)", 0, CROP)]
CASES = [(f"{key}/{bd}", f"{label}, {bd} bit", bd, o, win) for bd in (10, 8) for key, label, o, win in SHAPES]
SETUP_COPIES = 1                                            # reformat calls in front of the cases: the 8-bit sources


def moved(bd, win):
    w, h = W - win[0] - win[1], H - win[2] - win[3]
    return 2 * planes(bd, w, h)


def run(a):
    import torch

    from openhevc_amd.engine import Engine
    eng = Engine(0)
    n = a.pictures
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(13)
    yuv = torch.randint(0, 1024, (n, H * 3 // 2, W), dtype=torch.int16, device=dev, generator=g).view(torch.uint16)
    main10, _ = eng.pics_import(yuv, "planar", bit_depth=10, chroma_format_idc=1)
    del yuv
    srcs = {10: main10, 8: eng.pics_reformat(main10, bit_depth=8)}      # SETUP_COPIES
    eng.sync()
    dsts, copies = {}, {}
    for key, label, bd, o, win in CASES:
        src = srcs[bd]
        shape = (bd, bool(o & 4), win)
        if shape not in dsts:
            dsts[shape], _ = eng.pics_orient(src, o, window=win)            # warm-up, allocates
        else:
            eng.pics_orient(src, o, window=win, out=dsts[shape])
        dst = dsts[shape]
        if bd not in copies:
            copies[bd] = eng.pics_reformat(src)                             # warm-up, allocates
        else:
            eng.pics_reformat(src, out=copies[bd])
        cp = copies[bd]
        eng.sync()
        if o == 3:                                          # a half turn of a half turn is the picture
            back, _ = eng.pics_orient(dst[:2], 3)
            assert all(c.plane[k].differing == 0 for c in eng.pics_compare(src[:2], back, ssim=False) for k in range(3))
            for pid in back:
                eng.pic_free(pid)

        def orient():
            eng.pics_orient(src, o, window=win, out=dst)

        def copy():
            eng.pics_reformat(src, out=cp)

        def timed(fn):
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            eng.sync()
            return (time.perf_counter() - t0) / a.reps * 1e3

        ms = {"orient": [], "copy": []}
        for _ in range(a.rounds):
            ms["orient"].append(timed(orient))
            ms["copy"].append(timed(copy))
        med = {k: statistics.median(v) for k, v in ms.items()}
        best = {k: min(v) for k, v in ms.items()}
        nbytes, cbytes = moved(bd, win), 2 * planes(bd)
        print(json.dumps({"case": key, "what": label, "pictures": n, "orient_ms_median": round(med["orient"], 4),
                          "orient_ms_min": round(best["orient"], 4), "copy_ms_median": round(med["copy"], 4),
                          "copy_ms_min": round(best["copy"], 4), "bytes": n * nbytes, "copy_bytes": n * cbytes,
                          "orient_TBps": round(n * nbytes / (med["orient"] * 1e-3) / 1e12, 2),
                          "time_per_byte_to_copy": round((med["orient"] / nbytes) / (med["copy"] / cbytes), 3),
                          "time_per_byte_to_copy_min": round((best["orient"] / nbytes) / (best["copy"] / cbytes), 3)}), flush=True)
    eng.close()


def summarize(a):
    """kernel times of a rocprofv3 --kernel-trace --stats run of this tool: each case's orientation dispatches beside the copy's of the
    same sources, median and minimum, and the time per byte relative to the copy"""
    paths = sorted(glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        sys.exit(f"no *kernel_trace.csv under {a.summarize}")
    rows = sorted(csv.DictReader(open(paths[-1])), key=lambda r: int(r["Start_Timestamp"]))

    def find(kernel):
        return [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows if kernel in r["Kernel_Name"]]
    per_case = 1 + a.reps * a.rounds                        # the warm-up and the timed calls, in the order of CASES
    halves = sum(1 for c in CASES if c[3] == 3)             # the check of the half turn: one more orientation dispatch behind its warm-up
    ot, cp = find("::orient_"), find("reformat_kernel<")[SETUP_COPIES:]
    if len(ot) != len(CASES) * per_case + halves or len(cp) != len(CASES) * per_case:
        sys.exit(f"{len(ot)} orientation and {len(cp)} copy dispatches: not {len(CASES)} cases of 1 + {a.reps} x {a.rounds}; pass the run's "
                 "--pictures (at most 64), --reps and --rounds")
    n = a.pictures
    print(f"# {os.path.relpath(paths[-1], a.summarize)}: {n} pictures {W}x{H} per call; per byte: (orient time / orient bytes) / (copy time / copy bytes)")
    print(f"# {'case':48s} {'calls':>5s} {'med us':>8s} {'min us':>8s} {'MB/call':>8s} {'TB/s':>5s} | {'copy med us':>11s} {'MB/call':>8s} {'TB/s':>5s} | "
          f"{'per byte, med':>13s} {'min':>6s}")
    at = 0
    for i, (key, label, bd, o, win) in enumerate(CASES):
        mine = ot[at:at + per_case + (o == 3)]
        at += len(mine)
        if o == 3:
            del mine[1]                                     # the check's dispatch on two pictures
        v, c = sorted(t for _, t in mine), sorted(t for _, t in cp[i * per_case:(i + 1) * per_case])
        m, lo, cm, cmin = v[len(v) // 2], v[0], c[len(c) // 2], c[0]
        nbytes, cbytes = moved(bd, win), 2 * planes(bd)
        r, rmin = (m / nbytes) / (cm / cbytes), (lo / nbytes) / (cmin / cbytes)
        print(f"  ({key:5s}) {label:42s} {len(v):5d} {m:8.1f} {lo:8.1f} {n * nbytes / 1e6:8.1f} {n * nbytes / (m * 1e-6) / 1e12:5.2f} | {cm:11.1f} "
              f"{n * cbytes / 1e6:8.1f} {n * cbytes / (cm * 1e-6) / 1e12:5.2f} | {r:13.3f} {rmin:6.3f}")
        print(f"#       kernels: {mine[0][0]}; {cp[i * per_case][0]}")


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
