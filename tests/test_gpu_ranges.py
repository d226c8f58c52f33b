"""Byte-range reads from block-indexed streams on a real MI355X (-m gpu): zh_uncompress_ranges and
zh_plan_uncompress_ranges (zippy_amd/csrc/zh_ranges.hip).  Streams and indexes are the engine's own compress_blocks
(held equal to the oracle's by tests/test_gpu_parity.py); a range's expected bytes are the slice of the original input.
The shared cases are tests/ranges_cases.py's, as under the emulator (tests/test_emu_ranges.py)."""
import random

import pytest

import oracle
import ranges_cases as rc
import synth

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


@pytest.fixture(scope="module")
def make(eng):
    return rc.make_engine(eng)


def test_gpu_ranges_shapes(eng, make):
    rc.check_shapes(eng, make)


def test_gpu_ranges_formats_and_levels(eng, make):
    rc.check_formats(eng, make)


def test_gpu_ranges_clip_alignment(eng, make):
    rc.check_clip_alignment(eng, make)


def test_gpu_ranges_crafted_streams(eng):
    rc.check_crafted(eng)


def test_gpu_ranges_failures(eng, make):
    rc.check_damaged_block(eng, make)
    rc.check_moved_entry(eng, make)
    rc.check_bad_index_of_one_stream(eng, make)
    rc.check_small_slot(eng, make)


def test_gpu_ranges_call_errors(eng, make):
    rc.check_call_errors(eng, make)
    rc.check_plan_refuses_other_calls(eng, make)


def test_gpu_ranges_upload_accounting(eng, make):
    rc.check_upload_accounting(eng, make)


def test_gpu_ranges_4mib_blocks(eng, make):
    """two blocks of 4 MiB and one of 1 MiB: edge blocks of 4 MiB, clips of 256 pieces and more"""
    src = synth.gen_batch("mix", 1, 9 * MIB)[0].tobytes()
    blob, idx = make(src, 1, oracle.dfGzip, 4 * MIB)
    assert [e[1] for e in idx] == [0, 4 * MIB, 8 * MIB, 9 * MIB]
    ranges = [(0, 4 * MIB - 1, 2), (0, 1, 9 * MIB - 2)]
    rc.check_call(eng, [src], [blob], [idx], ranges)
    assert eng.debug_range_stats()[1:] == (1, 4)  # block 1 of the long range in place; four edges
    rc.check_call(eng, [src], [blob], [idx], ranges[:1])
    assert eng.debug_range_stats()[1:] == (0, 2)
    doff, dcap, size = rc.slots_for([2, 9 * MIB - 2], lead=5)
    lens, sts, stats = rc.run_plan(eng, [src], [blob], [idx], ranges, doff, dcap, size, runs=2)
    assert sts == [0, 0] and stats == (0, 1, 4)


@pytest.fixture(scope="module")
def batch64(eng, make):
    bufs = synth.gen_batch("mix", 64, 1 << 18)
    srcs = [bufs[i].tobytes() for i in range(64)]
    made = [make(srcs[i], (1, -1)[i % 2], oracle.dfGzip, rc.BB) for i in range(64)]
    return srcs, [m[0] for m in made], [m[1] for m in made]


def test_gpu_ranges_2048_ranges_of_64_streams(eng, batch64):
    srcs, streams, indexes = batch64
    rng = random.Random(20261018)
    ranges = [(rng.randrange(64), rng.randrange(1 << 18), rng.randrange(1, 100001)) for _ in range(2048)]
    rc.check_call(eng, srcs, streams, indexes, ranges)
    up, in_place, via_scratch = eng.debug_range_stats()
    S, U = rc.spans_of(indexes, [len(x) for x in streams], ranges)
    assert U <= up <= S + 64 * len(ranges)
    assert in_place > 0 and 2048 <= via_scratch <= 4096


def test_gpu_ranges_plan_runs_twice(eng, batch64):
    """the same plan into a destination that is poisoned again in between: the same lengths, statuses and bytes"""
    srcs, streams, indexes = batch64
    rng = random.Random(7)
    ranges = [(rng.randrange(64), rng.randrange(1 << 18), rng.randrange(1, 100001)) for _ in range(256)]
    lengths = [len(rc.want_slice(srcs[s], off, n)) for s, off, n in ranges]
    doff, dcap, size = rc.slots_for(lengths, lead=9)
    lens, sts, _ = rc.run_plan(eng, srcs, streams, indexes, ranges, doff, dcap, size, runs=2)
    assert sts == [0] * 256 and lens == lengths


def test_gpu_ranges_scratch_groups(eng, make, monkeypatch):
    src = rc.mix(rc.SHAPE_SIZE)
    blob, idx = make(src, 1, oracle.dfGzip, rc.BB)
    ranges = rc.straddling_ranges(64, len(src))
    want = rc.check_call(eng, [src], [blob], [idx], ranges)
    monkeypatch.setenv("ZH_SCRATCH_MB", "1")
    assert rc.check_call(eng, [src], [blob], [idx], ranges) == want
    assert eng.debug_range_stats()[1:] == (0, 128)


def test_gpu_ranges_contract_mode_streams(eng, make):
    """streams of the parallel BestSpeed parse (other bytes than zippy's, the same index semantics) read back by range"""
    src = rc.mix(rc.SHAPE_SIZE)
    eng.set_l1_parse(1)
    try:
        blob, idx = make(src, 1, oracle.dfGzip, rc.BB)
    finally:
        eng.set_l1_parse(-1)
    assert [e[1] for e in idx] == list(range(0, rc.SHAPE_SIZE, rc.BB)) + [rc.SHAPE_SIZE]
    rc.check_both(eng, [src], [blob], [idx], rc.shape_ranges())


def test_gpu_ranges_api(eng):
    from zippy_amd import api
    from zippy_amd.common import ZippyError
    src, blob, idx = rc.seven_blocks(rc.make_engine(eng))
    assert api.read_range(blob, idx, 3 * rc.BB - 7, 100) == src[3 * rc.BB - 7:3 * rc.BB + 93]
    damaged = bytearray(blob)
    at = (idx[3][0] // 8 + idx[4][0] // 8) // 2
    damaged[at] ^= 0xff
    damaged[at + 1] ^= 0xff
    with pytest.raises(ZippyError):
        api.read_range(bytes(damaged), idx, 3 * rc.BB + 5, 100)
    outs, sts = api.uncompress_ranges([bytes(damaged)], [idx], [(0, 3 * rc.BB + 5, 100), (0, 5, 100)])
    assert sts[0] != 0 and outs[0] is None and (sts[1], outs[1]) == (0, src[5:105])
