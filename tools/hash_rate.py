"""Rate of the picture hashes on the GPU: 32 pictures of 3840x2160 Main 10 4:2:0 (796 MB of packed planes) hashed in one call —
oh_pics_hash CRC (hash_type 1) and checksum (2), and oh_pics_md5 for comparison.  Host wall time per call (each call ends with a wait
for the engine stream; it includes the job hand-over and the launches).  Kernel times: run it under
    rocprofv3 --kernel-trace --stats -d OUTDIR -o hash -- python tools/hash_rate.py
in a run of its own (crc_kernel / checksum_kernel + hash_combine_kernel, md5_kernel)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openhevc_amd import frame as F                                          # noqa: E402
from openhevc_amd.engine import Engine                                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--md5-reps", type=int, default=2)
    a = ap.parse_args()
    p = F.pic_params(3840, 2160, bit_depth=10, chroma_format_idc=1)
    eng = Engine(0)
    rng = np.random.default_rng(1)
    pids = []
    for k in range(a.pictures):
        hp = F.HostPic(p)
        for c in range(3):
            v = hp.visible(c)
            v[...] = rng.integers(0, 1024, v.shape, dtype=v.dtype)
        pid = eng.pic_alloc(p)
        eng.pic_upload(pid, hp)
        pids.append(pid)
    eng.sync()
    nbytes = a.pictures * sum(hp.visible(c).nbytes for c in range(3))
    res = {"pictures": a.pictures, "geometry": "3840x2160 10 bit 4:2:0", "bytes": nbytes}

    def timed(fn, reps):
        fn()                                                  # warm-up: code objects, staging and device buffers
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps

    for t, name in ((1, "crc"), (2, "checksum")):
        s = timed(lambda: eng.pics_hash(pids, t), a.reps)
        res[name + "_call_ms"] = round(s * 1e3, 3)
        res[name + "_call_GBps"] = round(nbytes / s / 1e9, 1)
    s = timed(lambda: eng.pics_md5(pids), a.md5_reps)
    res["md5_call_ms"] = round(s * 1e3, 3)
    res["md5_call_GBps"] = round(nbytes / s / 1e9, 3)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
