#!/usr/bin/env python3
"""v1 zip reading end to end, host buffers in, verified entries out: ONE zh_zip_read_batch call (ZipArchive.open of
ziparchives_v1.nim) against ONE zh_zip_open_all_batch call (openZipArchive + extractAll of ziparchives.nim) on the same
images, in the same process, at the C ABI (readers closed inside the timed region).  Prints one JSON line.

    W1  256 archives of 16 x 64 KiB G-mix entries (writeZipArchive's layout, BestSpeed: both readers accept it)
    W2  16 archives of 4 x 64 MiB

    python tools/bench_zip_read.py [--reps 5] [--warmup 1] [--only W1,W2] [--no-trace] [--out FILE]

Every timing is the median of --reps runs after --warmup runs; min, max and the spread (max - min) / median are
reported next to it.  There is no pass mark: the two calls do different work (v1 reads every image byte once more per
scan pass and verifies lengths).  Unless --no-trace, the v1 call runs once more per workload with ZH_TRACE=1: what it
prints is stored under "trace", and the scan's two kernels (each between two HIP events) are set against the bytes
they read: "scan_count_pass" (every image byte once) with its GB/s, "scan_write_pass" (only the 16 KiB groups that
hold a hit).
"""
import argparse
import ctypes as c
import json
import os
import random
import re
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
    ap.add_argument("--only", default="W1,W2")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # torch's bundled HIP runtime first, as in the tests
    import synth
    from zippy_amd import api
    eng = api.engine()
    lib, h = eng.lib, eng._h

    def call(fn, images):
        n = len(images)
        srcs = (c.c_void_p * n)(*[c.cast(c.c_char_p(b), c.c_void_p) for b in images])
        lens = (c.c_size_t * n)(*[len(b) for b in images])
        readers, sts = (c.c_void_p * n)(), (c.c_int32 * n)()

        def run():
            assert fn(h, srcs, lens, n, readers, sts) == 0 and not any(sts), list(sts)[:8]
            total = 0
            blen = c.c_size_t()
            for r in readers:
                lib.zh_zip_data(r, c.byref(blen))
                total += blen.value
                lib.zh_zip_close(r)
            return total
        return run

    only = args.only.split(",")
    work = {}
    pool = synth.gen_batch("mix", 1, 64 << 20)[0].tobytes()
    if "W1" in only:
        rng = random.Random(42)
        archives = []
        for t in range(256):
            ents = []
            for i in range(16):
                at = rng.randrange(len(pool) - 65536)
                ents.append(("t%03d/d%d/f%02d.bin" % (t, i % 4, i), pool[at:at + 65536]))
            archives.append(ents)
        outs, sts = eng.write_zips(archives, 1)
        assert sts == [0] * 256
        work["W1_256x16x64KiB"] = outs
    if "W2" in only:
        outs, sts = eng.write_zips([[("big/%d.bin" % i, pool[i:] + pool[:i]) for i in range(4)]] * 2, 1)
        assert sts == [0, 0]
        work["W2_16x4x64MiB"] = [outs[k % 2] for k in range(16)]
    res = {"tool": "tools/bench_zip_read.py", "reps": args.reps, "warmup": args.warmup}
    for name, images in work.items():
        v1, v2 = call(lib.zh_zip_read_batch, images), call(lib.zh_zip_open_all_batch, images)
        total = v1()
        v2()
        row = {"archives": len(images), "extracted_MiB": round(total / 2**20, 2),
               "archive_MiB": round(sum(map(len, images)) / 2**20, 2),
               "read_batch": timed(v1, args.reps, args.warmup), "open_all_batch": timed(v2, args.reps, args.warmup)}
        row["read_over_open_all"] = round(row["read_batch"]["median_s"] / row["open_all_batch"]["median_s"], 3)
        if not args.no_trace:
            row["trace"] = traced(v1)
            for ln in row["trace"]:
                m = re.search(r"scan kernel 1\s+([0-9.]+) ms \(HIP events; count pass: (\d+) bytes read\)", ln)
                if m:  # the pass that reads every image byte
                    ms, nbytes = float(m.group(1)), int(m.group(2))
                    row["scan_count_pass"] = {"ms": ms, "bytes": nbytes,
                                              "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
                m = re.search(r"scan kernel 2\s+([0-9.]+) ms \(HIP events; write pass: (\d+) hits, at most (\d+) bytes", ln)
                if m:  # the pass over the 16 KiB groups that hold a hit
                    row["scan_write_pass"] = {"ms": float(m.group(1)), "hits": int(m.group(2)),
                                              "bytes_at_most": int(m.group(3))}
        res[name] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
