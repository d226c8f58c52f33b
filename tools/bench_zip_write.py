#!/usr/bin/env python3
"""v1 zip writing (zh_zip_write_batch) end to end, host buffers in and out, against two baselines on the same
entries: zh_compress_batch_crc32 followed by assembly on the host with the restatement of writeZipArchive
(tests/zip_v1_writer_model.py, Python, fed the device's streams and CRC-32s), and the CPU oracle's compress() on
--threads host threads (its streams only; assembly is the same as the first baseline's).  Prints one JSON line.

    W1  64 archives of Bagnon-10.2.31.zip's contents (tests/golden/ziparchives)
    W2  100 000 entries of 1-4 KiB, as 2 archives of 50 000 (one archive holds 65535 entries at most: the EOCD's
        16-bit count; zh_zip_write_batch refuses more with ZH_ERR_ZIP_TOO_LARGE)
    W3  16 archives of 4 x 64 MiB synth entries (four distinct buffers, shared by the archives)

All at DefaultCompression (writeZipArchive's own level).

    python tools/bench_zip_write.py [--reps 3] [--scale 1.0] [--only W1,W2,W3] [--no-baseline] [--threads 16]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (zh_zip_write_kernel's row).
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def workloads(eng, scale):
    import synth
    reader = eng.open_zip(synth.fixture("ziparchives/Bagnon-10.2.31.zip"))
    files = [i for i, e in enumerate(reader.entries) if not e["is_directory"]]
    outs, _ = reader.extract_batch(files)
    got = dict(zip(files, outs))
    bagnon = [(e["path"], (got.get(i, b""), e["is_directory"], 0x6000, 0x5521)) for i, e in enumerate(reader.entries)]
    reader.close()
    w1 = [bagnon for _ in range(max(1, int(64 * scale)))]
    pool = synth.gen_batch("mix", 1, 16 << 20)[0].tobytes()
    rng = random.Random(42)
    w2 = [[], []]
    for i in range(max(2, int(100000 * scale))):
        k = rng.randrange(1024, 4097)
        at = rng.randrange(len(pool) - k + 1)
        w2[i & 1].append(("w2/d%03d/f%06d.bin" % (i % 512, i), (pool[at:at + k], False, i & 0xFFFF, 0x5521)))
    big = [b.tobytes() for b in synth.gen_batch("mix", 4, max(1 << 20, int((64 << 20) * scale)))]
    w3 = [[("a%02d/e%d.bin" % (t, j), (big[j], False, 0x6000, 0x5521)) for j in range(4)] for t in range(16)]
    return {"W1": w1, "W2": w2, "W3": w3}


def best(f, reps):
    t_best, out = 1e9, None
    for _ in range(reps):
        t = time.perf_counter()
        out = f()
        t_best = min(t_best, time.perf_counter() - t)
    return t_best, out


def compress_crc(eng, bufs, level):
    """zh_compress_batch_crc32 of `bufs` (raw deflate) -> (streams, crcs)"""
    n = len(bufs)
    srcs = (C.c_void_p * n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in bufs])
    dsts, dlens, sts, crcs = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int32 * n)(), (C.c_uint32 * n)()
    eng._check(eng.lib.zh_compress_batch_crc32(eng._h, srcs, lens, n, level, 3, dsts, dlens, sts, crcs))
    try:
        assert list(sts) == [0] * n
        return [C.string_at(dsts[i], dlens[i]) for i in range(n)], list(crcs)
    finally:
        for i in range(n):
            if dsts[i]:
                eng.lib.zh_free(dsts[i])


def assemble(zips, streams, crcs, level):
    """the model's archives from per-entry streams / CRCs given in entry order (non-empty entries only)"""
    import zip_v1_writer_model as zm
    it_s, it_c = iter(streams), iter(crcs)
    return [zm.image(z, level, deflate=lambda c, lv: next(it_s), crc32=lambda c: next(it_c)) for z in zips]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="entries / sizes x this (profiling runs: < 1)")
    ap.add_argument("--only", default="W1,W2,W3")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--threads", type=int, default=16, help="host threads of the oracle baseline")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # torch's bundled HIP runtime first, as in the tests
    import oracle
    from zippy_amd import api
    eng = api.engine()
    level = -1
    eng.write_zip([("warm", b"x" * 1000)])  # context, code objects
    res = {"tool": "tools/bench_zip_write.py", "scale": args.scale, "reps": args.reps, "level": level}
    for name, zips in workloads(eng, args.scale).items():
        if name not in args.only.split(","):
            continue
        prep = eng.prepare_zips(zips)
        eng.write_zips_prepared(prep, level)  # warm-up of this shape
        t_dev, (outs, sts) = best(lambda: eng.write_zips_prepared(prep, level), args.reps)
        assert sts == [0] * len(zips), (name, sorted(set(sts)))
        bufs = [v[0] for z in zips for _, v in z if len(v[0])]
        in_bytes = sum(len(b) for b in bufs)
        out_bytes = sum(len(o) for o in outs)
        row = {"archives": len(zips), "entries": sum(len(z) for z in zips), "input_GiB": round(in_bytes / 2**30, 4),
               "archive_GiB": round(out_bytes / 2**30, 4), "device_call_s": round(t_dev, 4),
               "device_input_GiBps": round(in_bytes / 2**30 / t_dev, 3)}
        if not args.no_baseline:
            compress_crc(eng, bufs[:1], level)
            t_cmp, (streams, crcs) = best(lambda: compress_crc(eng, bufs, level), args.reps)
            t_asm, imgs = best(lambda: assemble(zips, streams, crcs, level), 1)
            assert imgs == outs  # the same bytes both ways
            distinct = list({id(b): b for b in bufs}.values())  # (W3: its four buffers)
            t_or, _ = oracle.batch_mt(distinct, 0, level, oracle.dfDeflate, threads=args.threads)
            or_bytes = sum(len(b) for b in distinct)
            row.update({"compress_batch_crc32_s": round(t_cmp, 4), "host_assembly_s": round(t_asm, 4),
                        "compress_then_host_s": round(t_cmp + t_asm, 4),
                        "device_speedup_vs_compress_then_host": round((t_cmp + t_asm) / t_dev, 2),
                        "oracle_threads": args.threads, "oracle_input_MiB": round(or_bytes / 2**20, 1),
                        "oracle_cpu_GiBps": round(or_bytes / 2**30 / t_or, 4),
                        "oracle_cpu_s_for_all_input": round(in_bytes / (or_bytes / t_or), 3)})
        res[name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
