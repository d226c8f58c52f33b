#!/usr/bin/env python3
"""createZipArchive for many archives (zh_zip_create_batch) end to end, host buffers in and out, against a loop of
zh_zip_create -- one call an archive -- over the same archives.  zh_zip_create is the single-archive entry point as
it was before the batch call existed and is untouched by it, so the loop IS the behaviour a caller had before.
Prints one JSON line.

    W1  256 archives of 16 entries of 64 KiB synth `mix` (many small archives: what the batch call is for)
    W2  64 archives of Bagnon-10.2.31.zip's contents (tests/golden/ziparchives)
    W3  16 archives of 4 x 64 MiB synth entries (four distinct buffers, shared by the archives)

All at BestSpeed (createZipArchive's own level).  Both ways get their C arrays ready-made and are timed from the
first C call to the last byte copied into Python bytes; they alternate, `--reps` times each (default 5), after a
warm-up of each on the same shape.  Per workload: the median of either way, the loop's spread (max - min of its
repetitions: the run-to-run noise the comparison allows for), the ratio loop / batch, and
`batch_not_slower` = batch median <= loop median + loop spread.  The archives of the two ways are compared.

    python tools/bench_zip_create.py [--reps 5] [--scale 1.0] [--only W1,W2,W3]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (zh_zip_create_kernel's row); the
line's `kernel_image_bytes` is what that kernel writes in one batch call (every byte of every image, once).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T, D = 0x6000, 0x5521


def workloads(eng, scale):
    import synth
    small = [b.tobytes() for b in synth.gen_batch("mix", max(16, int(4096 * scale)), 65536)]
    w1 = [[("w1/a%03d/e%02d.bin" % (t, j), small[16 * t + j]) for j in range(16)] for t in range(len(small) // 16)]
    reader = eng.open_zip(synth.fixture("ziparchives/Bagnon-10.2.31.zip"))
    files = [i for i, e in enumerate(reader.entries) if not e["is_directory"]]
    outs, _ = reader.extract_batch(files)
    got = dict(zip(files, outs))
    bagnon = [(e["path"], got.get(i, b"")) for i, e in enumerate(reader.entries)]
    reader.close()
    w2 = [bagnon for _ in range(max(1, int(64 * scale)))]
    big = [b.tobytes() for b in synth.gen_batch("mix", 4, max(1 << 20, int((64 << 20) * scale)))]
    w3 = [[("a%02d/e%d.bin" % (t, j), big[j]) for j in range(4)] for t in range(16)]
    return {"W1": w1, "W2": w2, "W3": w3}


def prepare_loop(zips):
    """zh_zip_create's C arrays, one set an archive"""
    out = []
    for z in zips:
        n = len(z)
        names = [p.encode("utf-8", "surrogateescape") if isinstance(p, str) else bytes(p) for p, _ in z]
        blobs = [v for _, v in z]
        out.append((n, (C.c_char_p * n)(*names), (C.c_size_t * n)(*[len(x) for x in names]),
                    (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in blobs]),
                    (C.c_size_t * n)(*[len(b) for b in blobs]), names, blobs))
    return out


def run_loop(eng, prepared):
    outs = []
    for n, names, nlens, blobs, blens, _, _ in prepared:
        dst, dlen = C.c_void_p(), C.c_size_t()
        eng._check(eng.lib.zh_zip_create(eng._h, names, nlens, blobs, blens, n, T, D, C.byref(dst), C.byref(dlen)))
        try:
            outs.append(C.string_at(dst, dlen.value))
        finally:
            eng.lib.zh_free(dst)
    return outs


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="archives / sizes x this (rehearsals: < 1)")
    ap.add_argument("--only", default="W1,W2,W3")
    ap.add_argument("--no-loop", action="store_true", help="the batch call alone (profiling runs)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # torch's bundled HIP runtime first, as in the tests
    from zippy_amd import api
    eng = api.engine()
    eng.create_zips_one([("warm", b"x" * 1000)], T, D)  # context, code objects
    res = {"tool": "tools/bench_zip_create.py", "scale": args.scale, "reps": args.reps, "level": 1}
    for name, zips in workloads(eng, args.scale).items():
        if name not in args.only.split(","):
            continue
        prep_batch = eng.prepare_zips_v2(zips, T, D)
        prep_loop = prepare_loop(zips)
        outs, sts = eng.create_zips_prepared(prep_batch)  # warm-up of this shape, either way
        assert sts == [0] * len(zips), (name, sorted(set(sts)))
        t_batch, t_loop = [], []
        if not args.no_loop:
            assert run_loop(eng, prep_loop) == outs  # the same bytes both ways
        for _ in range(args.reps):
            t_batch.append(timed(lambda: eng.create_zips_prepared(prep_batch))[0])
            if not args.no_loop:
                t_loop.append(timed(lambda: run_loop(eng, prep_loop))[0])
        in_bytes = sum(len(v) for z in zips for _, v in z)
        out_bytes = sum(len(o) for o in outs)
        mb = statistics.median(t_batch)
        row = {"archives": len(zips), "entries": sum(len(z) for z in zips), "input_GiB": round(in_bytes / 2**30, 4),
               "archive_GiB": round(out_bytes / 2**30, 4), "kernel_image_bytes": out_bytes,
               "batch_s": [round(t, 5) for t in t_batch], "batch_median_s": round(mb, 5),
               "batch_input_GiBps": round(in_bytes / 2**30 / mb, 3)}
        if not args.no_loop:
            ml, spread = statistics.median(t_loop), max(t_loop) - min(t_loop)
            row.update({"loop_s": [round(t, 5) for t in t_loop], "loop_median_s": round(ml, 5),
                        "loop_spread_s": round(spread, 5), "loop_over_batch": round(ml / mb, 3),
                        "batch_not_slower": bool(mb <= ml + spread)})
        res[name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
