#!/usr/bin/env python3
"""zh_compress_stream_batch on one MI355X: what compressing streams piece by piece costs, host buffers in and out --

  1  --streams G-mix buffers of --size bytes at BestSpeed gzip, all fed side by side in pieces of 64 KiB and of 256 KiB,
     every piece with a sync flush and the last one finished, against one zh_compress_batch of the same buffers whole:
     GiB/s, calls, and the compressed size relative to the whole-buffer result -- the price of flushing and of no history
  2  --small streams fed ONE piece of 4 KiB each with a sync flush: the small-piece case, where the plan's fixed cost shows

A figure is one wall-clock run around the binding's calls (its copies of the results included) after a warm-up.  The
kernels' own times come from a further pass with ZH_TRACE=1, whose lines (HIP events around the plan's run and around
the consts and splice kernels) are read back from stderr and summed over the calls.  Not the headline bench (bench.py);
no number gates anything.  Prints one JSON line and, with --out, writes it to a file.

    python tools/bench_stream.py [--streams 1024] [--size 1048576] [--small 4096] [--out FILE]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SYNC, FINISH = 1, 2


def feed_all(eng, bufs, piece, level, fmt):
    """every buffer in pieces of `piece` bytes, one call a round of pieces -> (the streams, calls, seconds)"""
    n = len(bufs)
    rounds = max((len(b) + piece - 1) // piece for b in bufs)
    state, out = None, [[] for _ in range(n)]
    t = time.perf_counter()
    for r in range(rounds):
        last = r == rounds - 1
        outs, state, sts = eng.compress_stream_batch([b[r * piece:(r + 1) * piece] for b in bufs], state,
                                                     FINISH if last else SYNC, level, fmt, 0)
        assert not any(sts), sts
        for i in range(n):
            out[i].append(outs[i])
    dt = time.perf_counter() - t
    return [b"".join(o) for o in out], rounds, dt


def traced(fn):
    """fn() with ZH_TRACE=1 -> the sums of the 'plan' and 'splice' milliseconds of its stderr lines"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        os.environ["ZH_TRACE"] = "1"
        try:
            fn()
        finally:
            del os.environ["ZH_TRACE"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    pairs = re.findall(r"stream: plan ([0-9.]+) ms, splice ([0-9.]+) ms", text)
    return round(sum(float(p) for p, _ in pairs), 3), round(sum(float(s) for _, s in pairs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import synth
    from zippy_amd import api
    eng = api.engine()
    eng.set_gzip_fname_len(0)
    level, fmt = api.BestSpeed, api.dfGzip
    bufs = [b.tobytes() for b in synth.gen_batch("mix", a.streams, a.size)]
    raw = sum(len(b) for b in bufs)
    res = {"what": "zh_compress_stream_batch: %d G-mix buffers of %d bytes at BestSpeed gzip fed side by side in pieces "
                   "with sync flushes, against one zh_compress_batch of the same buffers; %d streams of one 4 KiB piece"
                   % (a.streams, a.size, a.small), "streams": a.streams, "stream_bytes": a.size}
    eng.compress_batch(bufs, level, fmt)  # the warm-up
    t = time.perf_counter()
    whole, sts = eng.compress_batch(bufs, level, fmt)
    dt = time.perf_counter() - t
    assert not any(sts)
    whole_bytes = sum(len(z) for z in whole)
    res["whole_batch"] = {"ms": round(dt * 1e3, 3), "GiBps": round(raw / dt / 2**30, 3), "compressed_bytes": whole_bytes}
    for piece in (65536, 262144):
        feed_all(eng, bufs[:64], piece, level, fmt)  # (the warm-up of this shape)
        zs, calls, dt = feed_all(eng, bufs, piece, level, fmt)
        assert eng.uncompress_batch(zs[:8], api.dfGzip)[0] == bufs[:8]
        size = sum(len(z) for z in zs)
        plan_ms, splice_ms = traced(lambda: feed_all(eng, bufs, piece, level, fmt))
        res["pieces_%d" % piece] = {"ms": round(dt * 1e3, 3), "GiBps": round(raw / dt / 2**30, 3), "calls": calls,
                                    "compressed_bytes": size, "size_vs_whole": round(size / whole_bytes, 4),
                                    "plan_kernels_ms": plan_ms, "splice_kernels_ms": splice_ms}
    small = [bufs[i % a.streams][(i // a.streams) * 4096:][:4096] for i in range(a.small)]
    one = lambda: eng.compress_stream_batch(small, None, SYNC, level, fmt, 0)
    one()
    t = time.perf_counter()
    outs, states, sts = one()
    dt = time.perf_counter() - t
    assert not any(sts)
    eng.compress_batch(small, level, fmt)  # (warmed like the streaming call)
    t = time.perf_counter()
    ws, sts = eng.compress_batch(small, level, fmt)
    dw = time.perf_counter() - t
    plan_ms, splice_ms = traced(one)
    res["small_pieces"] = {"streams": a.small, "piece_bytes": 4096, "ms": round(dt * 1e3, 3),
                           "GiBps": round(a.small * 4096 / dt / 2**30, 3), "compressed_bytes": sum(len(o) for o in outs),
                           "whole_batch_ms": round(dw * 1e3, 3), "whole_batch_compressed_bytes": sum(len(w) for w in ws),
                           "plan_kernels_ms": plan_ms, "splice_kernels_ms": splice_ms}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
