#!/usr/bin/env python3
"""zh_uncompress_resume_batch on one MI355X: what decoding streams as their bytes arrive costs, host buffers in and out --

  1  --members zlib-6 gzip members of --size bytes of G-mix, all fed side by side in pieces of 64 KiB and of 256 KiB
     (max_out = 4 x the piece, doubled for a stream that answers NEED_OUTPUT without progress), against one
     zh_uncompress_batch of the same members whole
  2  one zlib-6 stream of --big MiB in pieces of 8 MiB: one workgroup, the case this entry point does not serve

A figure is one wall-clock run around the binding's calls (its copies of the results included) after a warm-up of 1's
whole batch.  Not the headline bench (bench.py); no number gates anything.  Prints one JSON line and, with --out, writes
it to a file.

    python tools/bench_resume.py [--members 1024] [--size 1048576] [--big 256] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def gz(plain, wbits=31):
    c = zlib.compressobj(6, zlib.DEFLATED, wbits)
    return c.compress(plain) + c.flush()


def feed_all(eng, streams, piece, max_out):
    """every stream in pieces of `piece` bytes, one call a round of pieces -> (outputs' total, calls, seconds)"""
    n = len(streams)
    state, tail, pos, budget = [None] * n, [b""] * n, [0] * n, [max_out] * n
    why = [1] * n
    live = list(range(n))
    total = calls = 0
    t = time.perf_counter()
    while live:
        for i in live:
            if why[i] == 1:
                tail[i] += streams[i][pos[i]:pos[i] + piece]
                pos[i] += piece
        outs, used, states, whys, sts = eng.uncompress_resume_batch(
            [tail[i] for i in live], [state[i] for i in live], [budget[i] for i in live],
            [pos[i] >= len(streams[i]) for i in live])
        calls += 1
        nxt = []
        for k, i in enumerate(live):
            assert sts[k] == 0, (i, sts[k])
            total += len(outs[k])
            tail[i] = tail[i][used[k]:]
            state[i], why[i] = states[k], whys[k]
            if whys[k] == 2 and not outs[k]:
                budget[i] *= 2
            if whys[k] != 0:
                nxt.append(i)
        live = nxt
    return total, calls, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1024)
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--big", type=int, default=256, help="MiB of the one large stream")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import synth
    from zippy_amd import api
    eng = api.engine()
    plains = [b.tobytes() for b in synth.gen_batch("mix", a.members, a.size)]
    members = [gz(p) for p in plains]
    raw_bytes = sum(len(p) for p in plains)
    res = {"what": "zh_uncompress_resume_batch: %d zlib-6 gzip members of %d bytes fed side by side in pieces, against "
                   "one zh_uncompress_batch of the same members; one zlib-6 stream of %d MiB in pieces of 8 MiB"
                   % (a.members, a.size, a.big),
           "members": a.members, "member_bytes": a.size, "compressed_bytes": sum(len(m) for m in members)}
    eng.uncompress_batch(members, api.dfGzip)  # the warm-up
    t = time.perf_counter()
    outs, sts = eng.uncompress_batch(members, api.dfGzip)
    dt = time.perf_counter() - t
    assert all(s == 0 for s in sts) and outs[0] == plains[0]
    res["whole_batch"] = {"ms": round(dt * 1e3, 3), "GiBps": round(raw_bytes / dt / 2**30, 3)}
    for piece in (65536, 262144):
        total, calls, dt = feed_all(eng, members, piece, 4 * piece)
        assert total == raw_bytes
        res["pieces_%d" % piece] = {"ms": round(dt * 1e3, 3), "GiBps": round(raw_bytes / dt / 2**30, 3), "calls": calls}
    big_plain = b"".join(plains)[:a.big << 20]
    while len(big_plain) < a.big << 20:
        big_plain += big_plain[:(a.big << 20) - len(big_plain)]
    big = gz(big_plain, 15)
    total, calls, dt = feed_all(eng, [big], 8 << 20, 32 << 20)
    assert total == len(big_plain)
    res["one_stream"] = {"MiB": a.big, "compressed_bytes": len(big), "ms": round(dt * 1e3, 3),
                         "ms_per_MiB_in": round(dt * 1e3 / (len(big) / 2**20), 3),
                         "GiBps": round(len(big_plain) / dt / 2**30, 3), "calls": calls}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
