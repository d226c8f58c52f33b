#!/usr/bin/env python3
"""Tarball writing (zh_tar_create_batch) end to end, host buffers in and out, against two baselines on the same
bytes: the image assembled on the host by the restatement of writeTarball (tests/tar_writer_model.py, Python)
followed by eng.compress_batch, and the CPU oracle's compress() (W2, on a slice).  Prints one JSON line.

    W1  256 tarballs x 128 entries of 1-64 KiB, BestSpeed
    W2  1 tarball of 4096 x 256 KiB, DefaultCompression (writeTarball's own level)
    W3  1 tarball of 200 000 entries of 0-600 bytes, plain and BestSpeed

    python tools/bench_tar_create.py [--reps 3] [--scale 1.0] [--only W1,W2,W3] [--no-baseline]

Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (zh_tar_header_kernel's row).
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def workloads(scale):
    import synth
    pool = synth.gen_batch("mix", 1, 64 << 20)[0].tobytes()
    rng = random.Random(42)

    def entries(n, lo, hi, tag):
        out = []
        for i in range(n):
            k = rng.randrange(lo, hi + 1)
            at = rng.randrange(len(pool) - k + 1)
            out.append(("%s/d%03d/f%06d.bin" % (tag, i % 512, i), (pool[at:at + k], "0", 1700000000 + i)))
        return out

    w1 = [entries(max(1, int(128 * scale)), 1024, 65536, "t%d" % t) for t in range(256)]
    w2 = [entries(max(1, int(4096 * scale)), 262144, 262144, "w2")]
    w3 = [entries(max(1, int(200000 * scale)), 0, 600, "w3")]
    return {"W1": (w1, [1]), "W2": (w2, [-1]), "W3": (w3, ["plain", 1])}


def best(f, reps):
    t_best, out = 1e9, None
    for _ in range(reps):
        t = time.perf_counter()
        out = f()
        t_best = min(t_best, time.perf_counter() - t)
    return t_best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="entries per tarball x this (profiling runs: < 1)")
    ap.add_argument("--only", default="W1,W2,W3")
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # torch's bundled HIP runtime first, as in the tests
    import oracle
    import tar_writer_model as twm
    from zippy_amd import api
    from zippy_amd.common import TAR_PLAIN, dfGzip
    eng = api.engine()
    eng.set_gzip_fname_len(0)
    eng.create_tar([("warm", b"x" * 1000)], dfGzip, 1)  # context, code objects
    res = {"tool": "tools/bench_tar_create.py", "scale": args.scale, "reps": args.reps}
    for name, (tars, levels) in workloads(args.scale).items():
        if name not in args.only.split(","):
            continue
        prep = eng.prepare_tars(tars)
        imgs = [twm.image(t) for t in tars]
        img_bytes = sum(len(i) for i in imgs)
        n_entries = sum(len(t) for t in tars)
        for lv in levels:
            fmt, level = (TAR_PLAIN, 0) if lv == "plain" else (dfGzip, lv)
            eng.create_tars_prepared(prep, fmt, level)  # warm-up of this shape
            t_dev, (outs, sts) = best(lambda: eng.create_tars_prepared(prep, fmt, level), args.reps)
            assert sts == [0] * len(tars)
            if fmt == TAR_PLAIN:
                assert outs == imgs
            elif len(imgs[0]) <= 256 << 20:  # zippy's compress() of the image (the first tarball, by the oracle)
                assert outs[0] == oracle.compress(imgs[0], level, oracle.dfGzip, fname_len=0)
            row = {"tarballs": len(tars), "entries": n_entries, "image_GiB": round(img_bytes / 2**30, 4),
                   "level": lv, "device_call_s": round(t_dev, 4),
                   "device_image_GiBps": round(img_bytes / 2**30 / t_dev, 3)}
            if not args.no_baseline:
                t_asm, _ = best(lambda: [twm.image(t) for t in tars], 1)
                if fmt == TAR_PLAIN:
                    t_cmp = 0.0
                else:
                    eng.compress_batch(imgs[:1], level, dfGzip)
                    t_cmp, (bouts, bsts) = best(lambda: eng.compress_batch(imgs, level, dfGzip), args.reps)
                    assert bouts == outs
                row.update({"host_assembly_s": round(t_asm, 4), "host_compress_batch_s": round(t_cmp, 4),
                            "host_total_s": round(t_asm + t_cmp, 4),
                            "host_image_GiBps": round(img_bytes / 2**30 / (t_asm + t_cmp), 3),
                            "device_speedup_vs_host": round((t_asm + t_cmp) / t_dev, 2)})
                if name == "W2":  # the CPU oracle on a slice of the image
                    sl = imgs[0][:32 << 20]
                    t_or, _ = best(lambda: oracle.compress(sl, level, oracle.dfGzip, fname_len=0), 1)
                    row["oracle_cpu_slice_MiB"] = len(sl) >> 20
                    row["oracle_cpu_GiBps"] = round(len(sl) / 2**30 / t_or, 4)
            res["%s_%s" % (name, lv)] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
