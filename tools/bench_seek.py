#!/usr/bin/env python3
"""Seek indexes for foreign streams on one MI355X, at sizes a user would run (host calls, wall clock, best of --steps):

  batch     index build of N x 1 MiB zlib-6 gzip members (zh_seek_index_batch, span 1 MiB, data not downloaded and
            downloaded) against zh_uncompress_batch of the same batch: the difference is what recording the points,
            gathering the windows and the per-interval CRCs cost
  single    one large zlib-6 stream: the index build (one workgroup: the segment-wise decoder records nothing), the
            whole stream read back through the index (every interval on its own) against zh_uncompress of it (the
            segment-wise path)
  ranges    random ranges of that stream through the index against decoding the whole stream and slicing; the
            uploaded bytes

Not the headline bench (bench.py).  Prints one JSON line and, with --out, writes it to a file.

    python tools/bench_seek.py [--members 1024] [--mib 256] [--ranges 4096] [--len 65536] [--span 0] [--steps 3] [--out FILE]
"""
import argparse
import json
import os
import random
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def deflate(data, level, wbits):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits)
    return c.compress(data) + c.flush()


def best(fn, steps):
    out, t = None, None
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        t = dt if t is None else min(t, dt)
    return out, round(t, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1024)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--len", type=int, default=65536)
    ap.add_argument("--span", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import synth
    from zippy_amd import api

    torch.cuda.init()
    eng = api.engine()
    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "span": args.span or (1 << 20)}

    # ---- a batch of members ----
    bufs = [b.tobytes() for b in synth.gen_batch("mix", args.members, 1 << 20)]
    members = [deflate(b, 6, 31) for b in bufs]
    (outs, sts), t_unc = best(lambda: eng.uncompress_batch(members, api.dfGzip), args.steps)
    assert all(s == 0 for s in sts) and outs[-1] == bufs[-1]
    (blobs, sts), t_idx = best(lambda: eng.seek_index_batch(members, api.dfGzip, args.span), args.steps)
    assert all(s == 0 for s in sts)
    (_, sts, data), t_idx_data = best(lambda: eng.seek_index_batch(members, api.dfGzip, args.span, want_data=True), args.steps)
    assert all(s == 0 for s in sts) and data[-1] == bufs[-1]
    res["batch"] = {"members": args.members, "member_bytes": 1 << 20, "compressed_bytes": sum(map(len, members)),
                    "uncompress_batch_ms": t_unc, "seek_index_batch_ms": t_idx, "seek_index_batch_with_data_ms": t_idx_data,
                    "index_bytes": sum(map(len, blobs))}
    del outs, data

    # ---- one large stream ----
    src = b"".join(bufs[:args.mib] if args.mib <= len(bufs) else [b.tobytes() for b in synth.gen_batch("mix", args.mib, 1 << 20)])
    stream = deflate(src, 6, 15)
    (out, t_unc1) = best(lambda: eng.uncompress(stream, api.dfZlib), args.steps)
    assert out == src
    (blob, t_build) = best(lambda: api.seek_index(stream, api.dfZlib, args.span), max(1, args.steps - 1))
    (whole, t_whole) = best(lambda: api.seek_read_range(stream, blob, 0, len(src)), args.steps)
    assert whole == src
    res["single"] = {"bytes": len(src), "compressed_bytes": len(stream), "uncompress_ms": t_unc1, "seek_index_ms": t_build,
                     "whole_read_through_index_ms": t_whole, "index_bytes": len(blob),
                     "points": (len(blob) - 64) // 32 if len(blob) < 64 + 32 * 4096 else None}
    del whole

    # ---- random ranges ----
    rng = random.Random(1)
    ranges = [(0, rng.randrange(len(src) - args.len), args.len) for _ in range(args.ranges)]
    ((outs, sts), t_ranges) = best(lambda: eng.seek_read_ranges([stream], [blob], ranges), args.steps)
    assert all(s == 0 for s in sts) and all(o == src[r[1]:r[1] + r[2]] for o, r in zip(outs[:64], ranges))
    up, _, intervals = eng.debug_range_stats()

    def slicing():
        whole = eng.uncompress(stream, api.dfZlib)
        return [whole[o:o + n] for _, o, n in ranges]
    (_, t_slice) = best(slicing, args.steps)
    res["ranges"] = {"ranges": args.ranges, "range_bytes": args.len, "seek_read_ranges_ms": t_ranges,
                     "uncompress_and_slice_ms": t_slice, "uploaded_bytes": up, "intervals_decoded": intervals}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
