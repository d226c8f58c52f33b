#!/usr/bin/env python3
"""Random access into one block-indexed stream on one MI355X: one buffer (default 256 MiB of G-mix) compressed with
32 KiB blocks at BestSpeed, then 4096 random ranges of 64 KiB read three ways --

  host call     zh_uncompress_ranges: host stream in, the ranges' bytes out (upload of the touched blocks only)
  ranges plan   zh_plan_uncompress_ranges: the stream resident in HBM, the ranges into device slots (HIP events)
  today's way   what a caller had to do before: uncompress_indexed of the WHOLE stream on the same box, then slice

Not the headline bench (bench.py).  Prints one JSON line and, with --out, writes it to a file.

    python tools/bench_ranges.py [--mib 256] [--block 32768] [--ranges 4096] [--len 65536] [--steps 3] [--out FILE]
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--block", type=int, default=32768)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--len", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    import torch
    import synth
    from zippy_amd import api
    from zippy_amd._binding import Engine

    size = args.mib << 20
    host = synth.gen_batch("mix", args.mib, 1 << 20).reshape(-1)
    src = host.tobytes()
    stream = torch.cuda.current_stream()
    eng = Engine(api.LIB_PATH, stream=stream.cuda_stream)
    eng.set_gzip_fname_len(0)
    blob, index = eng.compress_blocks(src, api.BestSpeed, api.dfGzip, args.block)
    rng = random.Random(20261018)
    ranges = [(0, rng.randrange(size - args.len), args.len) for _ in range(args.ranges)]

    def wall(fn):
        best = None
        for _ in range(args.steps):
            t = time.perf_counter()
            res = fn()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        return best * 1e3, res

    # the host call (the Python binding's copies of the results are inside the time, as they are for today's way)
    host_ms, (outs, sts) = wall(lambda: eng.uncompress_ranges([blob], [index], ranges))
    assert sts == [0] * len(ranges)
    for (_, off, n), out in zip(ranges[:64], outs[:64]):
        assert out == src[off:off + n]
    uploaded, in_place, via_scratch = eng.debug_range_stats()
    del outs

    # today's way, host buffers: the whole stream up, the whole output down, then the slices
    def whole():
        back = eng.uncompress_indexed(blob, index, api.dfGzip)
        return [back[off:off + n] for _, off, n in ranges]
    whole_ms, sl = wall(whole)
    assert sl[0] == src[ranges[0][1]:ranges[0][1] + args.len]
    del sl

    # resident in HBM: the ranges plan against the indexed plan of the whole stream
    d_comp = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_back = torch.empty(size, dtype=torch.uint8, device="cuda")
    slot = (args.len + 255) // 256 * 256
    d_slots = torch.empty(slot * len(ranges), dtype=torch.uint8, device="cuda")
    rplan = eng.plan_uncompress_ranges([0], [len(blob)], [index], ranges, [slot * r for r in range(len(ranges))],
                                       [args.len] * len(ranges))
    rplan.set_profiling(True)
    uplan = eng.plan_uncompress_indexed(0, len(blob), 0, size, index, api.dfGzip)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    rplan.run(d_comp.data_ptr(), d_slots.data_ptr())
    uplan.run(d_comp.data_ptr(), d_back.data_ptr())
    lens, rsts = rplan.results()
    assert rsts == [0] * len(ranges) and lens == [args.len] * len(ranges)
    _, off0, n0 = ranges[1]
    assert d_slots[slot:slot + n0].cpu().numpy().tobytes() == src[off0:off0 + n0]
    tr = tu = 0.0
    kms = {}
    for _ in range(args.steps):
        ev[0].record(stream)
        rplan.run(d_comp.data_ptr(), d_slots.data_ptr())
        ev[1].record(stream)
        uplan.run(d_comp.data_ptr(), d_back.data_ptr())
        ev[2].record(stream)
        ev[2].synchronize()
        tr += ev[0].elapsed_time(ev[1])
        tu += ev[1].elapsed_time(ev[2])
        run_ms = {}  # (zh_inflate_kernel is launched twice a group: in place, then into scratch)
        for name, ms in rplan.kernel_times():
            run_ms[name] = run_ms.get(name, 0.0) + ms
        for name, ms in run_ms.items():
            kms.setdefault(name, []).append(ms)
    out = {
        "workload": "1 x %d MiB G-mix, %d-byte blocks, BestSpeed gzip; %d random ranges of %d bytes" %
                    (args.mib, args.block, args.ranges, args.len),
        "compressed_bytes": len(blob),
        "range_bytes": args.ranges * args.len,
        "host_call_ms": round(host_ms, 3),
        "host_whole_stream_then_slice_ms": round(whole_ms, 3),
        "uploaded_bytes": uploaded,
        "blocks_in_place": in_place,
        "blocks_via_scratch": via_scratch,
        "plan_ranges_ms": round(tr / args.steps, 4),
        "plan_whole_stream_indexed_ms": round(tu / args.steps, 4),
        "plan_ranges_kernels_ms": {k: round(sum(v) / len(v), 4) for k, v in kms.items() if k != "end"},
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
