#!/usr/bin/env python3
"""Zip reading end to end, host buffers in, extracted entries out: ONE zh_zip_open_all_batch call against a loop of
zh_zip_open + zh_zip_extract_batch (all file indices) + zh_zip_close per archive on the same images, in the same
process, at the C ABI (readers closed and results freed inside the timed region).  Prints one JSON line.

    W1  256 archives of 16 x 64 KiB G-mix entries (createZipArchive's layout, BestSpeed)
    W2  64 copies of the reference's fixture tests/golden/ziparchives/Bagnon-10.2.31.zip (a few hundred small entries)
    W3  16 archives of 4 x 64 MiB

    python tools/bench_zip_open.py [--reps 5] [--warmup 1] [--only W1,W2,W3] [--batch-only] [--trace]

Every timing is the median of --reps runs after --warmup runs; min, max and the spread (max - min) / median are
reported next to it.  --trace runs the batch call once more per workload with ZH_TRACE=1 and stores what it prints --
the call's phases (wall clock), the walk's kernels between two HIP events, the plan's kernels from
zh_plan_set_profiling -- under "trace".
"""
import argparse
import ctypes as c
import json
import os
import random
import statistics
import sys
import tempfile
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


def traced(f):
    """f() once with ZH_TRACE=1, -> the lines it wrote to stderr"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["ZH_TRACE"] = "1"
        try:
            f()
        finally:
            os.environ.pop("ZH_TRACE")
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return [ln.strip() for ln in tmp.read().decode(errors="replace").splitlines() if ln.startswith("[zh]")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="W1,W2,W3")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # torch's bundled HIP runtime first, as in the tests
    import synth
    from zippy_amd import api
    from zippy_amd._binding import ZipEntry
    eng = api.engine()
    lib, h = eng.lib, eng._h

    def batch(images):
        n = len(images)
        srcs = (c.c_void_p * n)(*[c.cast(c.c_char_p(b), c.c_void_p) for b in images])
        lens = (c.c_size_t * n)(*[len(b) for b in images])
        readers, sts = (c.c_void_p * n)(), (c.c_int32 * n)()

        def run():
            assert lib.zh_zip_open_all_batch(h, srcs, lens, n, readers, sts) == 0 and not any(sts)
            total = 0
            blen = c.c_size_t()
            for r in readers:
                lib.zh_zip_data(r, c.byref(blen))
                total += blen.value
                lib.zh_zip_close(r)
            return total
        return run

    def loop(images):
        def run():
            total = 0
            for b in images:
                r = c.c_void_p()
                assert lib.zh_zip_open(b, len(b), c.byref(r)) == 0
                e = ZipEntry()
                idx = []
                for i in range(lib.zh_zip_num_entries(r)):
                    lib.zh_zip_entry_at(r, i, c.byref(e))
                    if not e.is_directory:
                        idx.append(i)
                m = len(idx)
                cidx, dsts = (c.c_size_t * m)(*idx), (c.c_void_p * m)()
                dlen, sts = (c.c_size_t * m)(), (c.c_int32 * m)()
                assert lib.zh_zip_extract_batch(h, r, cidx, m, dsts, dlen, sts) == 0 and not any(sts)
                total += sum(dlen)
                for d in dsts:
                    lib.zh_free(d)
                lib.zh_zip_close(r)
            return total
        return run

    only = args.only.split(",")
    work = {}
    if "W1" in only or "W3" in only:
        pool = synth.gen_batch("mix", 1, 64 << 20)[0].tobytes()
    if "W1" in only:
        rng = random.Random(42)
        tables = []
        for t in range(256):
            ents = []
            for i in range(16):
                at = rng.randrange(len(pool) - 65536)
                ents.append(("t%03d/d%d/f%02d.bin" % (t, i % 4, i), pool[at:at + 65536]))
            tables.append(ents)
        outs, sts = eng.create_zips(tables)
        assert sts == [0] * 256
        work["W1_256x16x64KiB"] = outs
    if "W2" in only:
        with open(os.path.join(ROOT, "tests", "golden", "ziparchives", "Bagnon-10.2.31.zip"), "rb") as f:
            work["W2_64xBagnon"] = [f.read()] * 64
    if "W3" in only:
        outs, sts = eng.create_zips([[("big/%d.bin" % i, pool[i:] + pool[:i]) for i in range(4)]] * 2)
        assert sts == [0, 0]
        work["W3_16x4x64MiB"] = [outs[k % 2] for k in range(16)]
    res = {"tool": "tools/bench_zip_open.py", "reps": args.reps, "warmup": args.warmup}
    for name, images in work.items():
        b = batch(images)
        total = b()
        row = {"archives": len(images), "extracted_MiB": round(total / 2**20, 2),
               "archive_MiB": round(sum(map(len, images)) / 2**20, 2), "batch": timed(b, args.reps, args.warmup)}
        if not args.batch_only:
            lp = loop(images)
            lp()
            row["loop"] = timed(lp, args.reps, args.warmup)
            row["loop_over_batch"] = round(row["loop"]["median_s"] / row["batch"]["median_s"], 3)
        if args.trace:
            row["trace"] = traced(b)
        res[name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
