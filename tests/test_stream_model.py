"""CPU-only, no engine: the model of zh_compress_stream_batch (tests/stream_model.py) held against what it must mean.
Every prefix that ends in a sync flush decodes, with Python's zlib, to exactly the bytes fed so far, and every
finished stream decodes whole with nothing left over; pieces that are multiples of the block size, fed with BLOCK and
finished, are byte for byte the oracle's compress_blocks of the whole -- and a piece that is no multiple is not; the
alignment family of tests/stream_cases.py reaches every case of the placing."""
import random
import zlib

import oracle
import stream_cases as sc
import stream_model as sm


def test_model_state_layout():
    assert sm.STATE.size == 64
    blob = sm.pack_state(2, -1, 65536, 5, 0x15, 0xdeadbeef, 0x1122334455, 0x66778899aa)
    assert blob[:8] == b"ZHCSTRM1" and blob[8:12] == b"\1\0\0\0" and blob[12] == 2 and blob[16:20] == b"\xff" * 4
    assert blob[20:24] == b"\0\0\1\0" and blob[24] == 1 and blob[28] == 5 and blob[32] == 0x15
    assert blob[36:40] == bytes.fromhex("efbeadde") and blob[40:45] == bytes.fromhex("5544332211")
    assert blob[48:53] == bytes.fromhex("aa99887766") and blob[56:] == bytes(8)
    assert sm.state_sound(blob) and not sm.state_sound(blob[:-1]) and not sm.state_sound(blob + b"\0")


def test_model_sync_prefixes_and_finished_streams_decode():
    rng = random.Random(5)
    syncs = 0
    for trial in range(24):
        level = (0, 1, 3, 6, -2)[trial % 5]
        fmt = sc.FORMATS[trial % 3]
        total = rng.randint(0, 200000)
        data = b"".join((sc.text, sc.rnd)[rng.randint(0, 1)](rng.randint(0, 50000), trial * 16 + j) for j in range(16))[:total]
        state, z, fed, at = None, b"", b"", 0
        d = zlib.decompressobj(sc.WBITS[fmt])
        got = b""
        while True:
            n = rng.choice((0, 0, 1, 7, rng.randint(0, 70000)))
            piece = data[at:at + n]
            at += len(piece)
            fl = sm.FINISH if at >= len(data) and rng.random() < 0.5 else rng.choice((sm.BLOCK, sm.SYNC))
            out, state, st = sm.step(state, piece, fl, level, fmt, 32768)
            assert st == sm.OK
            fed += piece
            got += d.decompress(out)
            if fl == sm.SYNC:
                assert got == fed
                syncs += 1
            if fl == sm.FINISH:
                assert got == fed and d.eof and not d.unused_data and state is None
                break
            assert sm.state_sound(state) and sm.State(state).total_in == len(fed)
    assert syncs > 40


def test_model_identity_and_its_negative_control():
    whole = sc.text(50000, 11) + sc.rnd(40000, 11) + sc.text(80000, 12) + b"tail"
    differ = 0
    for level in (1, 6, 0, -2):
        unit = 65535 if level == 0 else 32768
        for fmt in sc.FORMATS:
            ref = oracle.compress_blocks(whole, level, fmt, 32768)[0]
            for mult in (1, 2, 3):
                cuts = [whole[at:at + unit * mult] for at in range(0, len(whole), unit * mult)]
                outs = sm.run(cuts, [sm.BLOCK] * (len(cuts) - 1) + [sm.FINISH], level, fmt, 32768)
                assert b"".join(outs) == ref, (level, fmt, mult)
            # a piece that is no multiple of the block size: still the same data, not the same bytes
            cuts = [whole[:unit + 1000], whole[unit + 1000:]]
            z = b"".join(sm.run(cuts, [sm.BLOCK, sm.FINISH], level, fmt, 32768))
            sc.decodes(z, fmt, whole)
            differ += z != ref
    assert differ >= 9  # (level 0 may agree where the stored chunks happen to fall alike)
    # block_bytes 0 is the reference's own compress()
    z = b"".join(sm.run([whole], [sm.FINISH], 1, sm.DF_GZIP, 0, fname_len=3))
    assert z == oracle.compress(whole, 1, sm.DF_GZIP, 3)


def test_model_alignment_family_reaches_every_case():
    chains = sc.align_chains((sm.DF_DEFLATE,))
    streams = sc.run_chains(sc.ModelEngine(), chains)
    assert sc.align_tags(chains) == sc.ALIGN_ALL, sc.ALIGN_ALL - sc.align_tags(chains)
    for ch, z in zip(chains, streams):
        sc.decodes(z, ch.fmt, ch.whole)
    # ... a family of 40 does not (so the 100 are not for show), and the emulator's few reach the same
    forty = sc.align_chains((sm.DF_DEFLATE,), ns=range(1, 41))
    sc.run_chains(sc.ModelEngine(), forty)
    print("a family of 40 misses", sorted(sc.ALIGN_ALL - sc.align_tags(forty)))
    assert sc.align_tags(forty) < sc.ALIGN_ALL
    few = sc.align_chains((sm.DF_DEFLATE,), ns=sc.align_cover())
    sc.run_chains(sc.ModelEngine(), few)
    assert sc.align_tags(few) == sc.ALIGN_ALL and len(sc.align_cover()) <= 16


def test_model_case_families_decode():
    eng = sc.ModelEngine()
    sc.check_stored(eng)
    sc.check_empty(eng)
    sc.check_lengths(eng, (1, 0, -2), (sm.DF_ZLIB,))
    sc.check_bad_states(eng)
    sc.check_batch33(eng)
