#!/usr/bin/env python3
"""zh_gzip_read_batch on one MI355X: what not knowing the members' boundaries costs, host buffers in and out --

  1  --images x --members zlib-6 members of 1 MiB of G-mix through zh_gzip_read_batch, against zh_uncompress_batch of
     the same members handed over already split (as .gz files of one member): the difference is the scan, the sizing
     pass and the walk; its phases under ZH_TRACE from one more run
  2  the same data as a BGZF file (zh_bgzf_write_batch at level 6) through zh_bgzf_read_batch, for scale
  3  one image of --warc members of ~ 10 KiB, the WARC shape
  4  one image that is a single member of --big MiB: the worst case of the sizing pass, one workgroup
  5  the first once more for the member list alone (no data comes down)

Every figure is the best of three wall-clock runs around the binding's call (its copies of the results included) after
one warm-up.  Not the headline bench (bench.py).  Prints one JSON line and, with --out, writes it to a file.

    python tools/bench_gzip.py [--images 64] [--members 16] [--warc 100000] [--big 256] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gz_member(plain, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(plain) + c.flush()


def best_of_3(fn):
    res = fn()  # the warm-up
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        res = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(min(ts), 3), res


def traced(fn):
    """the [zh] lines one run of fn writes to stderr under ZH_TRACE"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.environ["ZH_TRACE"] = "1"
        try:
            os.dup2(tmp.fileno(), 2)
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["ZH_TRACE"]
        tmp.seek(0)
        return [line.strip() for line in tmp.read().decode(errors="replace").splitlines() if line.startswith("[zh]")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--warc", type=int, default=100000)
    ap.add_argument("--big", type=int, default=256)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import synth
    from zippy_amd import api
    from zippy_amd._binding import Engine

    eng = Engine(api.LIB_PATH, stream=torch.cuda.current_stream().cuda_stream)
    eng.set_gzip_fname_len(0)
    size = 1 << 20
    out = {"method": "best of 3 wall-clock runs after one warm-up, host buffers in and out"}

    def emit():
        line = json.dumps(out)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return line

    # 1, 2, 5: images of members of 1 MiB (64 distinct members, dealt round)
    plains = [b.tobytes() for b in synth.gen_batch("mix", 64, size)]
    gz = [gz_member(p) for p in plains]
    pick = [[(i * args.members + k) % 64 for k in range(args.members)] for i in range(args.images)]
    images = [b"".join(gz[j] for j in row) for row in pick]
    split = [gz[j] for row in pick for j in row]
    multi_ms, (outs, sts, mems) = best_of_3(lambda: eng.gzip_read_batch(images))
    assert sts == [0] * len(images) and outs[0] == b"".join(plains[j] for j in pick[0]) and len(mems[-1]) == args.members
    stats = eng.debug_gzip_stats()
    del outs
    split_ms, (outs, sts) = best_of_3(lambda: eng.uncompress_batch(split, api.dfGzip))
    assert sts == [0] * len(split) and outs[1] == plains[pick[0][1]]
    del outs
    list_ms, (_, sts, _) = best_of_3(lambda: eng.gzip_read_batch(images, want_data=False))
    assert sts == [0] * len(images)
    out.update({
        "1_workload": "%d images of %d zlib-6 members of 1 MiB of G-mix (%d members, %d image bytes)" %
                      (args.images, args.members, len(split), sum(map(len, images))),
        "1_gzip_read_batch_ms": multi_ms,
        "1_uncompress_batch_of_the_members_split_ms": split_ms,
        "1_price_of_the_boundaries_ms": round(multi_ms - split_ms, 3),
        "1_price_of_the_boundaries_percent": round(100.0 * (multi_ms - split_ms) / split_ms, 2),
        "1_candidates": stats[0], "1_speculative_bytes": stats[1], "1_frontier_rounds": stats[2],
        "1_phases_zh_trace": traced(lambda: eng.gzip_read_batch(images)),
        "5_members_only_ms": list_ms,
    })
    print(emit(), flush=True)
    srcs = [b"".join(plains[j] for j in row) for row in pick]
    files, sts = eng.bgzf_compress_batch(srcs, 6, 0)
    assert sts == [0] * len(srcs)
    bgzf_ms, (outs, sts) = best_of_3(lambda: eng.bgzf_uncompress_batch(files))
    assert sts == [0] * len(srcs) and outs[0] == srcs[0]
    out.update({"2_bgzf_read_batch_same_data_ms": bgzf_ms, "2_bgzf_file_bytes": sum(map(len, files))})
    del outs, srcs, files, images, split
    print(emit(), flush=True)

    # 3: the WARC shape
    small = [gz_member(plains[j % 64][(j * 10007) % (size - 12000):][:9000 + 97 * (j % 23)]) for j in range(256)]
    warc = b"".join(small[j % 256] for j in range(args.warc))
    warc_ms, (outs, sts, mems) = best_of_3(lambda: eng.gzip_read_batch([warc]))
    assert sts == [0] and len(mems[0]) == args.warc
    stats = eng.debug_gzip_stats()
    out.update({"3_workload": "one image of %d members of ~ 10 KiB (%d image bytes, %d data bytes)" %
                              (args.warc, len(warc), len(outs[0])),
                "3_gzip_read_batch_ms": warc_ms, "3_candidates": stats[0], "3_speculative_bytes": stats[1],
                "3_frontier_rounds": stats[2], "3_phases_zh_trace": traced(lambda: eng.gzip_read_batch([warc]))})
    del outs, warc
    print(emit(), flush=True)

    # 4: one member of --big MiB
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    big = b"".join(c.compress(plains[j % 64]) for j in range(args.big)) + c.flush()
    big_ms, (outs, sts, mems) = best_of_3(lambda: eng.gzip_read_batch([big]))
    assert sts == [0] and len(mems[0]) == 1 and len(outs[0]) == args.big * size
    del outs
    one_ms, (outs, sts) = best_of_3(lambda: eng.uncompress_batch([big], api.dfGzip))
    assert sts == [0]
    out.update({"4_workload": "one image that is a single zlib-6 member of %d MiB (%d image bytes)" % (args.big, len(big)),
                "4_gzip_read_batch_ms": big_ms, "4_uncompress_batch_ms": one_ms,
                "4_phases_zh_trace": traced(lambda: eng.gzip_read_batch([big]))})
    print(emit(), flush=True)


if __name__ == "__main__":
    main()
