"""The names zh_plan_kernel_times reports, pinned for every kind of plan: tests/test_emu_kernel_times.py (fiber
emulator) and tests/test_gpu_kernel_times.py (MI355X) run each plan of collect() once with profiling on and hold the
list of names against EXPECTED -- same names, same order, same number of entries, the second stream's kernels last.
bench.py's collect_kernel_times, tools/kprof.py and zip_extract's trace read these lists.  Only names and order are
checked: the emulator's events are stubs that return 0 ms.
(A sizing run -- the count-only pass -- has no row: the binding does not expose it on a plan.)"""
import contextlib
import os

import synth
from ranges_cases import DeviceBuf

GZIP, ZLIB, DEFLATE = 1, 2, 3  # zippy's dfGzip / dfZlib / dfDeflate
SIZE = 40000  # two fragments a buffer
CAP = 65536

_L1 = ["zh_l1_match_kernel", "zh_huffman_kernel", "zh_layout_kernel", "zh_emit_kernel"]
_ASIDE = ["zh_checksum_pieces_kernel", "zh_checksum_combine_kernel"]
_CHAIN = ["zh_chain_prev_kernel", "zh_chain_walk_kernel", "zh_chain_select_kernel", "zh_frag_stats_kernel",
          "zh_huffman_kernel", "zh_layout_kernel", "zh_emit_kernel"]
_PAIR = ["zh_inflate_tokens_kernel", "zh_inflate_write_kernel"]
_VERIFY = ["zh_checksum_pieces_kernel", "zh_checksum_combine_kernel", "zh_verify_kernel"]

EXPECTED = {
    "compress level 1 gzip": _L1 + _ASIDE,
    "compress level 1 deflate": _L1,
    "compress level 6 zlib": _CHAIN + _ASIDE,
    "compress level 0 gzip": ["zh_huffman_kernel", "zh_layout_kernel", "zh_emit_kernel"] + _ASIDE,
    "compress level -2 gzip": _L1 + _ASIDE,
    "compress level 1 gzip, trailer late": _L1 + ["zh_trailer_kernel"] + _ASIDE,
    "uncompress 3 streams": ["zh_unwrap_kernel"] + _PAIR + _VERIFY,
    "uncompress 4 streams as two halves": ["zh_unwrap_kernel"] + _PAIR + [
        "zh_checksum_pieces_kernel", "(waiting for the other half)"] + _VERIFY + _PAIR,
    "uncompress 3 streams in token groups": ["zh_unwrap_kernel"] + 3 * _PAIR + _VERIFY,
    "uncompress 2 streams segment-wise": [
        "zh_unwrap_kernel", "zh_seg_find_kernel", "zh_seg_check_kernel", "zh_seg_substart_kernel",
        "zh_seg_tokens_kernel", "zh_seg_chain_kernel", "zh_seg_repair_kernel", "zh_seg_write_kernel",
        "zh_seg_windows_kernel", "zh_seg_finish_kernel"] + _PAIR + _VERIFY,
    "compress blocks level 6 gzip": _CHAIN + _ASIDE,
    "uncompress indexed": ["zh_unwrap_kernel", "zh_inflate_kernel", "zh_segments_reduce_kernel"] + _VERIFY,
    "uncompress ranges": ["zh_inflate_kernel", "zh_inflate_kernel", "zh_range_clip_kernel", "zh_ranges_reduce_kernel"],
}


@contextlib.contextmanager
def _env(**kv):
    """the switches a plan reads when it is made, put back afterwards"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _names(plan, d_src, d_dst):
    """one profiled run of `plan`, which is closed -> (names, lengths)"""
    try:
        plan.set_profiling(True)
        plan.run(d_src.p, d_dst.p)
        lens, sts = plan.results()
        assert all(s == 0 for s in sts), sts
        return [name for name, _ in plan.kernel_times()], lens
    finally:
        plan.close()


def collect(eng):
    """-> {case: the names kernel_times() gave}, the cases of EXPECTED in its order"""
    got, bufs = {}, []
    srcs = [b.tobytes() for b in synth.gen_batch("text", 3, SIZE, first_index=21)]
    off = [i * CAP for i in range(4)]
    d_src, d_dst = DeviceBuf(eng, b"".join(s.ljust(CAP, b"\0") for s in srcs)), DeviceBuf(eng, bytes(4 * CAP))
    d_big = DeviceBuf(eng, bytes(4 * 200000))
    bufs += [d_src, d_dst, d_big]
    try:
        def compress(case, level, fmt, **env):
            with _env(**env):
                plan = eng.plan_compress(off[:3], [SIZE] * 3, off[:3], [CAP] * 3, level, fmt)
            got[case], lens = _names(plan, d_src, d_dst)
            return lens
        gz_lens = compress("compress level 1 gzip", 1, GZIP)
        streams = [d_dst.read()[o:o + n] for o, n in zip(off, gz_lens)]
        compress("compress level 1 deflate", 1, DEFLATE)
        compress("compress level 6 zlib", 6, ZLIB)
        compress("compress level 0 gzip", 0, GZIP)
        compress("compress level -2 gzip", -2, GZIP)
        compress("compress level 1 gzip, trailer late", 1, GZIP, ZH_TRAILER_LATE="1")

        streams.append(streams[0])
        d_gz = DeviceBuf(eng, b"".join(s.ljust(CAP, b"\0") for s in streams))
        bufs.append(d_gz)

        def uncompress(case, n, cap, **env):
            with _env(**env):
                plan = eng.plan_uncompress(off[:n], [len(s) for s in streams[:n]], [i * cap for i in range(n)], [cap] * n, GZIP)
            got[case], lens = _names(plan, d_gz, d_big)
            assert lens == [SIZE] * n
        uncompress("uncompress 3 streams", 3, CAP)
        uncompress("uncompress 4 streams as two halves", 4, CAP, ZH_INFLATE_HALVES="4")
        # (slots of 200000 bytes: a stream's token region is then as large as its bits allow, and 1 MiB holds one)
        uncompress("uncompress 3 streams in token groups", 3, 200000, ZH_SCRATCH_MB="1")
        uncompress("uncompress 2 streams segment-wise", 2, CAP, ZH_SEG_MIN="2400", ZH_SEG_BYTES="600", ZH_SEG_SETUP="0")

        big = synth.gen_batch("text", 1, 100000, first_index=22)[0].tobytes()
        d_one, d_blk, d_out = DeviceBuf(eng, big), DeviceBuf(eng, bytes(131072)), DeviceBuf(eng, bytes(131072))
        bufs += [d_one, d_blk, d_out]
        plan = eng.plan_compress_blocks([0], [len(big)], [0], [131072], 6, GZIP, 32768)
        try:
            plan.set_profiling(True)
            plan.run(d_one.p, d_blk.p)
            (blob_len,), sts = plan.results()
            assert sts == [0]
            got["compress blocks level 6 gzip"] = [name for name, _ in plan.kernel_times()]
            index = plan.block_index(0)
        finally:
            plan.close()
        got["uncompress indexed"], lens = _names(
            eng.plan_uncompress_indexed(0, blob_len, 0, 131072, index, GZIP), d_blk, d_out)
        assert lens == [len(big)] and d_out.read()[:len(big)] == big
        # block 1 lies inside the range and is decoded in place, block 2 is cut by its end: an edge block
        got["uncompress ranges"], lens = _names(
            eng.plan_uncompress_ranges([0], [blob_len], [index], [(0, 32768, 32768 + 100)], [0], [131072]), d_blk, d_out)
        assert lens == [32768 + 100] and d_out.read()[:lens[0]] == big[32768:65536 + 100]
    finally:
        for b in bufs:
            b.free()
    assert list(got) == list(EXPECTED)
    return got
