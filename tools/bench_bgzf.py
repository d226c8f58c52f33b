#!/usr/bin/env python3
"""BGZF on one MI355X: 64 buffers of 1 MiB of G-mix at BestSpeed, three comparisons, host buffers in and out --

  write   zh_bgzf_write_batch against zh_compress_batch over the same data cut into the same 65 280-byte pieces as
          separate dfDeflate buffers (the way to do the same compression work without the feature)
  read    zh_bgzf_read_batch against zh_uncompress_batch_sized over the members' CDATA as separate raw streams
  ranges  2048 random ranges of up to 100 000 bytes (zh_bgzf_read_ranges) against zh_bgzf_read_batch of the whole files

One warm-up, then the median of --steps runs, the two sides of a comparison taking turns (wall clock around the
binding's call, its copies of the results included on both sides).  Not the headline bench (bench.py).  Prints one
JSON line and, with --out, writes it to a file.

    python tools/bench_bgzf.py [--bufs 64] [--steps 5] [--ranges 2048] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOCK = 65280


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bufs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--ranges", type=int, default=2048)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import synth
    from zippy_amd import api
    from zippy_amd._binding import Engine

    size = 1 << 20
    srcs = [b.tobytes() for b in synth.gen_batch("mix", args.bufs, size)]
    eng = Engine(api.LIB_PATH, stream=torch.cuda.current_stream().cuda_stream)
    eng.set_gzip_fname_len(0)

    def timed(*fns):
        """-> (median ms, last result) per function: one warm-up each, then the functions take turns"""
        res = [fn() for fn in fns]  # the warm-up
        ts = [[] for _ in fns]
        for _ in range(args.steps):
            for k, fn in enumerate(fns):
                t = time.perf_counter()
                res[k] = fn()
                ts[k].append((time.perf_counter() - t) * 1e3)
        out = [(statistics.median(t), r) for t, r in zip(ts, res)]
        return out if len(fns) > 1 else out[0]

    # write
    pieces = [s[o:o + BLOCK] for s in srcs for o in range(0, len(s), BLOCK)]
    (write_ms, (images, sts)), (pieces_ms, (cdatas, psts)) = timed(
        lambda: eng.bgzf_compress_batch(srcs, api.BestSpeed, 0),
        lambda: eng.compress_batch(pieces, api.BestSpeed, api.dfDeflate))
    assert sts == [0] * len(srcs) and psts == [0] * len(pieces)
    assert sum(len(x) for x in images) == sum(len(c) + 26 for c in cdatas) + 28 * len(srcs)

    # read
    hints = [len(p) for p in pieces]
    (read_ms, (back, sts)), (raw_ms, (outs, psts, _)) = timed(
        lambda: eng.bgzf_uncompress_batch(images),
        lambda: eng.uncompress_batch_sized(cdatas, api.dfDeflate, hints))
    assert sts == [0] * len(srcs) and back == srcs
    assert psts == [0] * len(pieces) and outs[0] == pieces[0] and outs[-1] == pieces[-1]
    del outs, back

    # ranges
    indexes, sts, eofs = eng.bgzf_index_batch(images)
    assert sts == [0] * len(srcs) and eofs == [1] * len(srcs)
    rng = random.Random(20261019)
    ranges = [(rng.randrange(len(srcs)), rng.randrange(size), rng.randrange(1, 100001)) for _ in range(args.ranges)]
    ranges_ms, (outs, sts) = timed(lambda: eng.bgzf_read_ranges(images, indexes, ranges))
    assert sts == [0] * len(ranges)
    for (t, off, n), out in zip(ranges[:64], outs[:64]):
        assert out == srcs[t][off:off + n]
    uploaded, in_place, via_scratch = eng.debug_range_stats()
    index_ms, _ = timed(lambda: eng.bgzf_index_batch(images))

    out = {
        "workload": "%d x 1 MiB G-mix, BestSpeed, members of %d bytes; %d random ranges of up to 100000 bytes" %
                    (args.bufs, BLOCK, args.ranges),
        "steps": args.steps,
        "image_bytes": sum(len(x) for x in images),
        "members": len(pieces) + len(srcs),
        "bgzf_write_ms": round(write_ms, 3),
        "pieces_compress_ms": round(pieces_ms, 3),
        "write_over_pieces": round(write_ms / pieces_ms, 4),
        "bgzf_read_ms": round(read_ms, 3),
        "pieces_uncompress_sized_ms": round(raw_ms, 3),
        "read_over_pieces": round(read_ms / raw_ms, 4),
        "bgzf_index_ms": round(index_ms, 3),
        "bgzf_ranges_ms": round(ranges_ms, 3),
        "ranges_over_whole_read": round(ranges_ms / read_ms, 4),
        "range_bytes": sum(len(o) for o in outs),
        "ranges_uploaded_bytes": uploaded,
        "ranges_members_in_place": in_place,
        "ranges_members_via_scratch": via_scratch,
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
