#!/usr/bin/env python3
"""Tarball reading end to end, host buffers in, readers out: zh_tar_open_batch against a loop of zh_tar_open calls on
the same images, in the same process, at the C ABI (the readers are closed inside the timed region; no Python objects
are built from them).  Prints one JSON line.

    W1  256 .tar.gz images of about 1 MiB uncompressed (16 entries of 64 KiB): one call against 256 calls
    W2  the reference's fixture, tarballs/libressl-3.4.2.tar.gz (21 MB, about 41 000 blocks), alone: the parallel walk
        costs some twenty short launches where the host's loop needs tens of microseconds

    python tools/bench_tar_open.py [--reps 9] [--warmup 2] [--only W1,W2] [--batch-only]

Every timing is the median of --reps runs after --warmup runs; min, max and the spread (max - min) / median are
reported next to it.  --batch-only skips the loop (for a run under `rocprofv3 --kernel-trace --stats`, whose zh_tar_*
rows are the walk's kernels; ZH_TRACE=1 prints the call's phases on stderr).
"""
import argparse
import ctypes as c
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(f, reps, warmup):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    med = statistics.median(ts)
    return {"median_s": round(med, 6), "min_s": round(min(ts), 6), "max_s": round(max(ts), 6),
            "spread": round((max(ts) - min(ts)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="W1,W2")
    ap.add_argument("--batch-only", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # torch's bundled HIP runtime first, as in the tests
    import synth
    from zippy_amd import api
    from zippy_amd.common import dfGzip
    eng = api.engine()
    eng.set_gzip_fname_len(0)
    lib, h = eng.lib, eng._h

    def batch(images):
        n = len(images)
        srcs = (c.c_void_p * n)(*[c.cast(c.c_char_p(b), c.c_void_p) for b in images])
        lens = (c.c_size_t * n)(*[len(b) for b in images])
        readers, sts = (c.c_void_p * n)(), (c.c_int32 * n)()

        def run():
            assert lib.zh_tar_open_batch(h, srcs, lens, n, readers, sts) == 0
            entries = sum(lib.zh_tar_num_entries(r) for r in readers)
            for r in readers:
                lib.zh_tar_close(r)
            return entries
        return run

    def loop(images):
        def run():
            entries = 0
            for b in images:
                r = c.c_void_p()
                assert lib.zh_tar_open(h, b, len(b), c.byref(r)) == 0
                entries += lib.zh_tar_num_entries(r)
                lib.zh_tar_close(r)
            return entries
        return run

    work = {}
    if "W1" in args.only.split(","):
        pool = synth.gen_batch("mix", 1, 64 << 20)[0].tobytes()
        rng = random.Random(42)
        tars = []
        for t in range(256):
            ents = []
            for i in range(16):
                at = rng.randrange(len(pool) - 65536)
                ents.append(("t%03d/d%d/f%02d.bin" % (t, i % 4, i), (pool[at:at + 65536], "0", 1700000000 + i)))
            tars.append(ents)
        outs, sts = eng.create_tars(tars, dfGzip, 1)
        assert sts == [0] * 256
        work["W1_256x1MiB_tgz"] = (outs, 256 * 16)
    if "W2" in args.only.split(","):
        work["W2_libressl_tgz"] = ([synth.fixture("tarballs/libressl-3.4.2.tar.gz")], 1743)
    res = {"tool": "tools/bench_tar_open.py", "reps": args.reps, "warmup": args.warmup}
    for name, (images, n_entries) in work.items():
        b = batch(images)
        assert b() == n_entries
        row = {"images": len(images), "entries": n_entries, "compressed_MiB": round(sum(map(len, images)) / 2**20, 2),
               "batch": timed(b, args.reps, args.warmup)}
        if not args.batch_only:
            lp = loop(images)
            assert lp() == n_entries
            row["loop"] = timed(lp, args.reps, args.warmup)
            row["loop_over_batch"] = round(row["loop"]["median_s"] / row["batch"]["median_s"], 3)
        res[name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
