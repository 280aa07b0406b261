"""Rate of oh_pics_unpack / oh_pics_pack on 32 frame-packed pictures of 3840x2160 4:2:0 per call, at 10 and 8 bit, both arrangements,
beside two parents in the same run:

  copy    oh_pics_reformat of the same sources to their own depth and format (a copy of the coded planes): time per destination byte
          relative to the copy.  A call that makes both views of full size writes twice the bytes of the packed pictures.
  chain   what the plain side-by-side case took before: oh_pics_orient cropping each half, then oh_pics_resize of each half by 2 : 1
          across — four launches and two intermediate pictures per packed picture.  It ignores the grid positions and is another filter,
          so only the time is compared: the ratio chain / unpack.

  half        both views of half size
  full        both views of full size, grid positions (0, 0) and (8, 0): the up-sampler
  full-flip   the same with view 1 stored mirrored
  one         view 0 alone at full size (what a 2D player asks for)
  quincunx    both views of full size from a quincunx arrangement
  pack        the half-size views back into a packed picture

Host wall time per call around `reps` calls and a wait for the engine stream; case and copy alternate, `rounds` times; the figures are
the median and the range of the rounds.

    python tools/packing_rate.py [--pictures 32] [--reps 3] [--rounds 5] [--depths 10,8]
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


def run(a):
    import torch

    from openhevc_amd import engine as E
    eng = E.Engine(0)
    n = a.pictures
    g = torch.Generator(device="cuda:0").manual_seed(25)

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        eng.sync()
        return (time.perf_counter() - t0) / a.reps * 1e3

    def stats(v):
        return round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)

    def pic_bytes(pid):
        p = eng._pic_params(pid)
        return p.width * p.height * 3 // 2 * (2 if p.bit_depth > 8 else 1)

    for bd in a.depths:
        yuv = torch.randint(0, 1 << bd, (n, H * 3 // 2, W), dtype=torch.int32, device="cuda:0", generator=g)
        t = yuv.to(torch.int16).view(torch.uint16) if bd > 8 else yuv.to(torch.uint8)
        src = eng.pics_import(t.contiguous(), "planar", bit_depth=bd, chroma_format_idc=1)[0]
        del yuv, t
        eng.sync()
        sp = eng._pic_params(src[0])
        cp = eng._alloc_like(sp, n)

        def copy():
            return eng.pics_reformat(src, out=cp)

        def measure(name, arr, case, dst_bytes, extra=None):
            case()
            copy()
            eng.sync()
            ms, cms = [], []
            for _ in range(a.rounds):
                ms.append(timed(case))
                cms.append(timed(copy))
            med, lo, hi = stats(ms)
            cmed, clo, chi = stats(cms)
            cb = n * pic_bytes(src[0])
            rec = {"case": name, "arrangement": arr, "bits": bd, "pictures": n, "image": [W, H], "ms_median": med, "ms_min": lo, "ms_max": hi,
                   "copy_ms_median": cmed, "copy_ms_min": clo, "copy_ms_max": chi, "dst_bytes": dst_bytes, "copy_dst_bytes": cb,
                   "GB_per_s_written": round(dst_bytes / med / 1e6, 1), "time_per_dst_byte_to_copy": round(med / dst_bytes / (cmed / cb), 2),
                   "time_per_dst_byte_to_copy_min": round(lo / dst_bytes / (chi / cb), 2),
                   "time_per_dst_byte_to_copy_max": round(hi / dst_bytes / (clo / cb), 2)}
            rec.update(extra or {})
            print(json.dumps(rec), flush=True)
            return ms

        for arr in ("side_by_side", "top_bottom"):
            grid = ((0, 0), (8, 0)) if arr == "side_by_side" else ((0, 0), (0, 8))
            plain = E.make_packing(arr, grid=grid)
            flipped = E.make_packing(arr, grid=grid, flip=(False, True))
            quincunx = E.make_packing(arr, quincunx=True)
            half = eng._alloc_like(plain.view_size(sp, False), 2 * n)
            full = eng._alloc_like(plain.view_size(sp, True), 2 * n)
            h2, f2 = (half[:n], half[n:]), (full[:n], full[n:])
            hb, fb = n * pic_bytes(half[0]), n * pic_bytes(full[0])
            measure("half", arr, lambda: eng.pics_unpack(src, plain, out=h2), 2 * hb)
            unpack_ms = measure("full", arr, lambda: eng.pics_unpack(src, plain, out=f2), 2 * fb)
            measure("full-flip", arr, lambda: eng.pics_unpack(src, flipped, out=f2), 2 * fb)
            measure("one", arr, lambda: eng.pics_unpack(src, plain, out=(f2[0], None)), fb)
            measure("quincunx", arr, lambda: eng.pics_unpack(src, quincunx, out=f2), 2 * fb)
            eng.pics_unpack(src, plain, out=h2)
            measure("pack", arr, lambda: eng.pics_pack(h2[0], h2[1], plain, out=cp), n * pic_bytes(cp[0]))
            if arr == "side_by_side":
                def chain():
                    for v in range(2):
                        eng.pics_orient(src, 0, window=(v * W // 2, (1 - v) * W // 2, 0, 0), out=h2[v])
                        eng.pics_resize(h2[v], (W, H), out=f2[v])

                chain_ms = measure("chain", arr, chain, 2 * fb)
                u, c = statistics.median(unpack_ms), statistics.median(chain_ms)
                print(json.dumps({"case": "chain / full", "arrangement": arr, "bits": bd, "unpack_ms_median": round(u, 3),
                                  "chain_ms_median": round(c, 3), "chain_to_unpack": round(c / u, 2),
                                  "chain_to_unpack_min": round(min(chain_ms) / max(unpack_ms), 2),
                                  "chain_to_unpack_max": round(max(chain_ms) / min(unpack_ms), 2)}), flush=True)
            for pid in half + full:
                eng.pic_free(pid)
        for pid in cp + src:
            eng.pic_free(pid)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depths", type=lambda s: [int(v) for v in s.split(",")], default=[10, 8])
    run(ap.parse_args())


if __name__ == "__main__":
    main()
