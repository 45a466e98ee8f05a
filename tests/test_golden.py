"""Committed fixtures: the oracle must reproduce them, and so must the device path.

  * tests/golden/{c1_seed1,multi_e7,repeat_rich}.npz, made by tests/golden/make_golden.py from the ORACLE: they freeze
    the oracle and the seeded generator
  * tests/golden/ref_*.npz, made by tests/golden/make_ref_golden.py from a build of THE REFERENCE'S OWN sources
    (oracle/_ref, `make -C oracle ref`): what the reference computed — no oracle/_ref is needed to check against them"""
import os

import numpy as np
import pytest

from tests.golden import make_ref_golden as mg
from tests.golden.make_golden import CASES, inputs, oracle_outputs

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_reproduces_the_fixture(name):
    want = np.load(os.path.join(HERE, name + ".npz"))
    got = oracle_outputs(CASES[name])
    for key in want.files:
        assert np.array_equal(want[key], got[key]), key
    if name == "c1_seed1":
        assert int(want["stats"][0]) == 1000 and 700 < int(want["stats"][1]) < 950  # config 1: most reads map
    if name == "repeat_rich":  # what SURVEY 8(c)(2) asks the repeat fixture to reach
        assert int(want["max_records_per_read"][0]) > 64 and int(want["reads_over_64_records"][0]) > 50
        assert int(want["strands_with_full_groups"][0]) > 100 and (want["in_text"] == ord("N")).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_reproduces_the_fixture(name):
    import hashlib
    from fem_amd import Device
    case = CASES[name]
    want = np.load(os.path.join(HERE, name + ".npz"))
    text, off, lens, bases, offs = inputs(case)
    dev = Device(0)
    try:
        dev.upload_reference([text[int(o):int(o) + int(l)] for o, l in zip(off, lens)])
        n, lookup, occ = dev.build_index(12, 3)
        assert np.array_equal(np.frombuffer(hashlib.sha256(lookup.tobytes() + occ.tobytes()).digest(), np.uint8),
                              want["index_sha256"])
        r = dev.map_batch(bases, offs, e=case["e"], a=case["a"])
        o, cand, ed, end = r.per_strand()
        assert np.array_equal(r.stats, want["stats"])
        assert np.array_equal(o, want["cand_off"]) and np.array_equal(cand, want["cands"])
        assert np.array_equal(ed, want["v_ed"])
        assert np.array_equal(end[ed != 0xFF], want["v_end"][want["v_ed"] != 0xFF])
        # the device mapping tail: same record text as the fixture's digest
        rec = dev.fetch_records()
        assert rec.n_records == int(want["n_records"][0])
        ops = "MID"

        def cigar(j):
            return "".join("%d%s" % (c >> 4, ops[c & 0xF]) for c in rec.cigar[rec.cigar_off[j]:rec.cigar_off[j + 1]]) or "*"

        sam = "".join("%d\t%d\t%d\t%d\t%s\t%d\t%s\n" % (
            r, int(rec.flag[j]), int(rec.tid[j]), int(rec.pos0[j]) + 1, cigar(j), int(rec.nm[j]),
            rec.md[rec.md_off[j]:rec.md_off[j + 1]].tobytes().decode())
            for r in range(case["n_reads"]) for j in range(int(rec.rec_begin[r]), int(rec.rec_begin[r + 1])))
        assert np.array_equal(np.frombuffer(hashlib.sha256(sam.encode()).digest(), np.uint8), want["records_sha256"])
    finally:
        dev.close()


@pytest.mark.parametrize("name", sorted(mg.CASES))
def test_oracle_reproduces_the_reference_fixture(name):
    case, want = mg.CASES[name], np.load(os.path.join(HERE, name + ".npz"))
    inp = mg.stored_inputs(name)
    assert mg.defined_region(inp, case["e"], case["a"])  # no read in a region where the reference has no defined answer
    got = mg.oracle_outcome(inp, case["e"], case["a"])
    assert int((got["r_flag"] & 0x8000).sum()) == 0
    for key in mg.STORED_KEYS:  # counters, candidates, (ed, end), every record field, the SAM and the index file's digests
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(mg.CASES))
def test_device_reproduces_the_reference_fixture(name):
    from fem_amd import Device
    case, want = mg.CASES[name], np.load(os.path.join(HERE, name + ".npz"))
    inp = mg.stored_inputs(name)
    assert mg.defined_region(inp, case["e"], case["a"])
    dev = Device(0)
    try:
        dev.upload_reference(inp.seqs)
        n, lookup, occ = dev.build_index(mg.K, mg.STEP)
        index_file = (np.array([mg.K, mg.STEP], "<i4").tobytes() + lookup.tobytes() + np.array([n], "<u8").tobytes() +
                      occ[:n].tobytes())  # the layout of save_index (src/index.c:136-168)
        assert np.array_equal(mg.sha(index_file), want["index_sha256"])
        batch = fo_batch(inp.reads)
        r = dev.map_batch(batch.bases, batch.off, e=case["e"], a=case["a"])
        o, cand, ed, end = r.per_strand()
        assert np.array_equal(r.stats, want["stats"])
        assert np.array_equal(o, want["cand_off"]) and np.array_equal(cand, want["cands"])
        assert np.array_equal(ed, want["v_ed"])
        assert np.array_equal(end[ed != 0xFF], want["v_end"][want["v_ed"] != 0xFF])
        rec = dev.fetch_records()
        for mine, theirs in (("rec_begin", "rec_off"), ("flag", "r_flag"), ("tid", "r_tid"), ("pos0", "r_pos"), ("nm", "r_nm"),
                             ("cigar_off", "cig_off"), ("cigar", "cig"), ("md_off", "md_off"), ("md", "md")):
            assert np.array_equal(getattr(rec, mine), want[theirs]), mine
    finally:
        dev.close()


def fo_batch(reads):
    from oracle import fem_oracle as fo
    return fo.ReadBatch(reads)
