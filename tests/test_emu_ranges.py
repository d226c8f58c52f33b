"""CPU-only: byte-range reads from block-indexed streams (zippy_amd/csrc/zh_ranges.hip: zh_uncompress_ranges,
zh_plan_uncompress_ranges) under the fiber emulator of tests/hipemu.  Streams and indexes come from
oracle.compress_blocks and tests/deflate_craft.py; a range's expected bytes are the slice of the original input.
The cases are tests/ranges_cases.py's, shared with tests/test_gpu_ranges.py."""
import pytest

import emu
import oracle
import ranges_cases as rc


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def test_emu_ranges_shapes(eng):
    rc.check_shapes(eng, rc.make_oracle)


def test_emu_ranges_formats_and_levels(eng):
    rc.check_formats(eng, rc.make_oracle)


def test_emu_ranges_clip_alignment(eng):
    rc.check_clip_alignment(eng, rc.make_oracle)


def test_emu_ranges_crafted_streams(eng):
    rc.check_crafted(eng)


def test_emu_ranges_damaged_block(eng):
    rc.check_damaged_block(eng, rc.make_oracle)


def test_emu_ranges_moved_entry(eng):
    rc.check_moved_entry(eng, rc.make_oracle)


def test_emu_ranges_bad_index_of_one_stream(eng):
    rc.check_bad_index_of_one_stream(eng, rc.make_oracle)


def test_emu_ranges_call_errors(eng):
    rc.check_call_errors(eng, rc.make_oracle)
    rc.check_plan_refuses_other_calls(eng, rc.make_oracle)


def test_emu_ranges_small_slot(eng):
    rc.check_small_slot(eng, rc.make_oracle)


def test_emu_ranges_upload_accounting(eng):
    rc.check_upload_accounting(eng, rc.make_oracle)


def test_emu_ranges_scratch_groups(eng, monkeypatch):
    """64 ranges that cut into two blocks of 32 KiB each -- 4 MiB of scratch -- with a budget of 1 MiB: groups of
    ranges take turns in the scratch, and return what the default budget returns"""
    src = rc.pattern(rc.SHAPE_SIZE)
    blob, idx = rc.make_oracle(src, 1, oracle.dfGzip, rc.BB)
    ranges = rc.straddling_ranges(64, len(src))
    want, want_sts = rc.check_call(eng, [src], [blob], [idx], ranges)
    assert eng.debug_range_stats()[1:] == (0, 128)
    monkeypatch.setenv("ZH_SCRATCH_MB", "1")
    got, sts = rc.check_call(eng, [src], [blob], [idx], ranges)
    assert (got, sts) == (want, want_sts)
    lengths = [r[2] for r in ranges]
    doff, dcap, size = rc.slots_for(lengths)
    rc.run_plan(eng, [src], [blob], [idx], ranges, doff, dcap, size, runs=2)  # (the plan, through the groups twice)


def test_emu_ranges_scratch_groups_are_made(eng, monkeypatch, capfd):
    """... and the small budget does make groups: the plan says so under ZH_TRACE"""
    src = rc.mix(rc.SHAPE_SIZE)
    blob, idx = rc.make_oracle(src, 1, oracle.dfGzip, rc.BB)
    monkeypatch.setenv("ZH_SCRATCH_MB", "1")
    monkeypatch.setenv("ZH_TRACE", "1")
    plan = eng.plan_uncompress_ranges([0], [len(blob)], [idx], rc.straddling_ranges(64, len(src)), [0] * 64, [1 << 20] * 64)
    plan.close()
    assert "scratch for 5 groups of ranges (64 ranges)" in capfd.readouterr().err


def test_emu_ranges_api(eng, monkeypatch):
    """api.read_range raises on a damaged block, api.uncompress_ranges hands the statuses out"""
    from zippy_amd import api
    from zippy_amd.common import ZippyError
    monkeypatch.setattr(api, "_engine", eng)
    src, blob, idx = rc.seven_blocks(rc.make_oracle)
    assert api.read_range(blob, idx, 3 * rc.BB + 5, 100) == src[3 * rc.BB + 5:3 * rc.BB + 105]
    assert api.read_range(blob, idx, len(src) + 1, 100) == b""
    damaged = bytearray(blob)
    at = (idx[3][0] // 8 + idx[4][0] // 8) // 2
    damaged[at] ^= 0xff
    damaged[at + 1] ^= 0xff
    with pytest.raises(ZippyError):
        api.read_range(bytes(damaged), idx, 3 * rc.BB + 5, 100)
    outs, sts = api.uncompress_ranges([bytes(damaged)], [idx], [(0, 3 * rc.BB + 5, 100), (0, 5, 100)])
    assert sts[0] != 0 and outs[0] is None and (sts[1], outs[1]) == (0, src[5:105])
