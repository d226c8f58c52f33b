#!/usr/bin/env python3
"""v1 tarball reading end to end, host buffers in, readers out: ONE zh_tar_read_batch call (Tarball.open of
tarballs_v1.nim) against ONE zh_tar_open_batch call (extractAll of tarballs.nim without the file system) on the same
images, in the same process, at the C ABI (readers closed inside the timed region).  Prints one JSON line.

    W1      256 tarballs of 16 x 64 KiB G-mix entries in writeTarball's layout, plain .tar images
    W1_gz   the same tarballs as .tar.gz (zh_tar_create_batch, BestSpeed)

    python tools/bench_tar_read.py [--reps 5] [--warmup 1] [--only W1,W1_gz] [--no-trace] [--out FILE]

Every timing is the median of --reps runs after --warmup runs; min, max and the spread (max - min) / median are
reported next to it.  There is no pass mark: the two calls do different work (the v1 walk steps over the trailer's zero
blocks one by one and parses its numbers strictly; extractAll checks every path and handles long names).  Unless
--no-trace, the v1 call runs once more per workload with ZH_TRACE=1: what it prints is stored under "trace".
"""
import argparse
import ctypes as c
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_zip_open import timed, traced  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="W1,W1_gz")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # torch's bundled HIP runtime first, as in the tests
    import synth
    from zippy_amd import api
    eng = api.engine()
    eng.set_gzip_fname_len(0)
    lib, h = eng.lib, eng._h

    def call(fn, images, *extra):
        n = len(images)
        srcs = (c.c_void_p * n)(*[c.cast(c.c_char_p(b), c.c_void_p) for b in images])
        lens = (c.c_size_t * n)(*[len(b) for b in images])
        readers, sts = (c.c_void_p * n)(), (c.c_int32 * n)()

        def run():
            assert fn(h, srcs, lens, *extra, n, readers, sts) == 0 and not any(sts), list(sts)[:8]
            total = entries = 0
            blen = c.c_size_t()
            for r in readers:
                lib.zh_tar_data(r, c.byref(blen))
                total += blen.value
                entries += lib.zh_tar_num_entries(r)
                lib.zh_tar_close(r)
            return total, entries
        return run

    only = args.only.split(",")
    pool = synth.gen_batch("mix", 1, 64 << 20)[0].tobytes()
    rng = random.Random(42)
    tarballs = []
    for t in range(256):
        ents = []
        for i in range(16):
            at = rng.randrange(len(pool) - 65536)
            ents.append(("t%03d/d%d/f%02d.bin" % (t, i % 4, i), (pool[at:at + 65536], "0", 1600000000 + i)))
        tarballs.append(ents)
    work = {}
    if "W1" in only:
        outs, sts = eng.create_tars(tarballs, -1, 1)
        assert sts == [0] * 256
        work["W1_256x16x64KiB_tar"] = outs
    if "W1_gz" in only:
        outs, sts = eng.create_tars(tarballs, 2, 1)
        assert sts == [0] * 256
        work["W1_256x16x64KiB_tar_gz"] = outs
    res = {"tool": "tools/bench_tar_read.py", "reps": args.reps, "warmup": args.warmup}
    for name, images in work.items():
        v1, v0 = call(lib.zh_tar_read_batch, images, None), call(lib.zh_tar_open_batch, images)
        total, entries = v1()
        assert (total, entries) == v0()
        row = {"tarballs": len(images), "entries": entries, "uncompressed_MiB": round(total / 2**20, 2),
               "image_MiB": round(sum(map(len, images)) / 2**20, 2),
               "read_batch": timed(v1, args.reps, args.warmup), "open_batch": timed(v0, args.reps, args.warmup)}
        row["read_over_open"] = round(row["read_batch"]["median_s"] / row["open_batch"]["median_s"], 3)
        if not args.no_trace:
            row["trace"] = traced(v1)
        res[name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
