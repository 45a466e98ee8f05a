"""The oracle and libfemhost against THE REFERENCE ITSELF, built from its own sources: oracle/_ref/FEM_ref is the
reference's command line and oracle/_ref/libfemref_fn.so its functions one read at a time (oracle/ref_fn.c), both compiled
from where the sources lie against a stand-in for the htslib declarations and a text-SAM writer (oracle/ref_standin*;
`make -C oracle ref`).  htslib does no mapping arithmetic, so everything but its text rendering is pinned here:

  * index files: `FEM_ref index` vs OracleIndex.save vs libfemhost's writer, byte for byte, seven seed shapes
  * stage by stage: candidates per strand with the count before the additional q-gram filter
    (generate_group_seeding_candidates), (ed, end) per candidate (verify_candidates: the 8-lane and the 32-bit Myers),
    CIGAR and MD per mapping (generate_alignment)
  * end to end: `FEM_ref map -t 1` vs the oracle's records, every SAM field and the five counters
  * the regions where the reference has no defined answer are fenced, not skipped: lower-case characters (it aborts —
    pinned read by read) and reads one seed short of the seed selection's table (it reads uninitialised memory — the
    oracle returns nothing there)

Without oracle/_ref (a checkout that never saw the reference's sources) what it returned stands in: tests/golden/ref_*.npz,
recorded by tests/golden/make_ref_golden.py.  With it, both are checked: the live build against the oracle, array by array,
and against the files, so that they cannot go stale.

Every comparison case asserts that none of its reads lies in an undefined region (comparable): the share of reads left
out of a comparison is zero."""
import os

import numpy as np
import pytest

from fem_amd import host
from oracle import fem_oracle as fo
from oracle import ref_fem
from tests.golden import make_ref_golden as mg

LIVE = ref_fem.available()
GOLDEN = os.path.dirname(os.path.abspath(mg.__file__))
_recorded = {}


def recorded(key):
    if not _recorded:
        _recorded.update(np.load(mg.RECORDED))
    return _recorded[key]


def comparable(inp, e, a, out):
    """The cap on excluded reads: no read of a comparison case in either undefined region."""
    assert mg.defined_region(inp, e, a), "upper-case ACGTN and every length at or above the formula's bound"
    assert all(len(r) >= mg.min_defined_length(e, a) for r in inp.reads)
    assert int((out["r_flag"] & 0x8000).sum()) == 0


def same_outcome(got, want, keys, what):
    for key in keys:
        assert np.array_equal(got[key], want[key]), "%s: %s" % (what, key)


def alignments_agree(inp, e, a, res):
    """generate_alignment of the reference for every mapping the oracle found, against the oracle's fo_align."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        fa, fq = inp.write(d)
        with ref_fem.RefFem(fa) as rf:
            assert rf.sequences() == [(n, len(s)) for n, s in zip(inp.names, inp.seqs)]
            rf.construct_index(mg.K, mg.STEP)
            assert rf.load_reads(fq, len(inp.reads)) == len(inp.reads)
            n = 0
            for r in range(len(inp.reads)):
                L = len(inp.reads[r])
                minus = fo.revcomp(inp.reads[r])
                for j in range(int(res.map_off[r]), int(res.map_off[r + 1])):
                    cand, direction, ed, end = int(res.m_cand[j]), int(res.m_dir[j]), int(res.m_ed[j]), int(res.m_end[j])
                    pos = cand & 0xFFFFFFFF
                    pattern = inp.seqs[cand >> 32][pos:pos + L + 2 * e + 2]
                    want = rf.align(e, r, direction, cand, ed, end)
                    assert fo.align(e, pattern, minus if direction else inp.reads[r], ed, end) == want, (r, j)
                    n += 1
            return n


# ------------------------------------------------------------------------------------------------ index files
@pytest.mark.parametrize("k,step", mg.INDEX_SHAPES)
def test_index_file_is_the_references(tmp_path, k, step):
    inp = mg.index_inputs()
    assert any(len(s) < k for s in inp.seqs) and any(b"N" in s for s in inp.seqs) and any(s != s.upper() for s in inp.seqs)
    idx = fo.OracleIndex(fo.Reference(inp.seqs), k, step)
    ours, hosts = str(tmp_path / "o.idx"), str(tmp_path / "h.idx")
    idx.save(ours)
    host.index_save(hosts, k, step, idx.lookup, idx.occ[:idx.n_occ])
    mine = open(ours, "rb").read()
    assert open(hosts, "rb").read() == mine
    assert np.array_equal(mg.sha(mine), recorded("index/%d_%d" % (k, step)))
    if LIVE:
        fa, _ = inp.write(str(tmp_path))
        theirs = str(tmp_path / "r.idx")
        ref_fem.cli_index(k, step, fa, theirs)
        assert open(theirs, "rb").read() == mine
        with ref_fem.RefFem(fa) as rf:  # ... and the tables themselves, before they are written
            rf.construct_index(k, step)
            rk, rstep, lookup, occ = rf.index_arrays()
            assert (rk, rstep) == (k, step) and np.array_equal(lookup, idx.lookup) and np.array_equal(occ, idx.occ[:idx.n_occ])
            rf.load_index(hosts)  # load_index of the reference reads our file back to the same tables
            rk, rstep, lookup, occ = rf.index_arrays()
            assert (rk, rstep) == (k, step) and np.array_equal(lookup, idx.lookup) and np.array_equal(occ, idx.occ[:idx.n_occ])


def test_reference_maps_from_an_index_file_of_ours(tmp_path):
    name = "ref_multi_ends"
    case, want = mg.CASES[name], np.load(os.path.join(GOLDEN, name + ".npz"))
    inp = mg.stored_inputs(name)
    idx = fo.OracleIndex(fo.Reference(inp.seqs), mg.K, mg.STEP)
    hosts = str(tmp_path / "h.idx")
    host.index_save(hosts, mg.K, mg.STEP, idx.lookup, idx.occ[:idx.n_occ])
    assert np.array_equal(mg.sha(open(hosts, "rb").read()), want["index_sha256"])  # the bytes FEM_ref wrote and read
    k, step, lookup, occ = host.index_load(hosts)
    assert (k, step) == (mg.K, mg.STEP) and np.array_equal(lookup, idx.lookup) and np.array_equal(occ, idx.occ[:idx.n_occ])
    if LIVE:
        fa, fq = inp.write(str(tmp_path))
        sam = str(tmp_path / "out.sam")
        r, counters = ref_fem.cli_map(case["e"], case["a"], fa, hosts, fq, sam)
        assert r.returncode == 0 and np.array_equal(counters, want["stats"])
        assert np.array_equal(mg.sha(open(sam, "rb").read()), want["sam_sha256"])


# ------------------------------------------------------------------------------------------------ stored-input cases
@pytest.mark.parametrize("name", sorted(mg.CASES))
def test_stored_case_stage_by_stage_and_end_to_end(name):
    case, want = mg.CASES[name], np.load(os.path.join(GOLDEN, name + ".npz"))
    inp = mg.stored_inputs(name)
    e, a = case["e"], case["a"]
    assert len(inp.reads) <= 500 and sum(len(s) for s in inp.seqs) <= 250_000
    got, res, _, _ = mg.oracle_outcome(inp, e, a, with_result=True)
    comparable(inp, e, a, got)
    same_outcome(got, want, mg.STORED_KEYS, "oracle vs the recorded reference")
    if LIVE:
        live = mg.reference_outcome(inp, e, a)
        same_outcome(live, want, mg.STORED_KEYS, "live reference vs its recording")
        assert live["sam_text"] == got["sam_text"]
        assert alignments_agree(inp, e, a, res) == int(want["stats"][4])


def test_stored_cases_reach_what_they_are_for():
    z = np.load(os.path.join(GOLDEN, "ref_repeat150_e7.npz"))
    per_strand, per_read = np.diff(z["cand_off"].astype(np.int64)), np.diff(z["rec_off"].astype(np.int64))
    full = per_strand[per_strand >= 8]
    assert len(full) > 100 and set((full % 8).tolist()) == set(range(8))  # the 8-lane Myers, and remainders of 1..7 after it
    assert (per_strand == 1).sum() > 20                                    # ... and strands with the 32-bit one alone
    assert int((per_read > 64).sum()) >= 10                                # klib's radix sort (above 64 records)
    reads = mg.stored_inputs("ref_repeat150_e7").reads
    assert sum(b"N" in r for r in reads) > 40 and (z["in_text"] == ord("N")).sum() > 100
    assert int((z["r_flag"] & 256).sum()) > 1000 and int((z["cig"] & 0xF == 1).sum()) > 0 and int((z["cig"] & 0xF == 2).sum()) > 0
    # reads at both ends of a sequence; candidates dropped and kept at the borders
    z, case = np.load(os.path.join(GOLDEN, "ref_multi_ends.npz")), mg.CASES["ref_multi_ends"]
    e, L = case["e"], case["L"]
    lens = z["in_lens"].astype(np.int64)
    assert (lens < L).sum() >= 2 and (lens < mg.K).sum() >= 1
    pos, tid = z["r_pos"].astype(np.int64), z["r_tid"].astype(np.int64)
    assert (pos <= 2 * e).sum() > 10 and (pos + L + 2 * e >= lens[tid]).sum() > 10
    assert 0 < int(z["stats"][1]) < int(z["stats"][0])  # some of the border reads are dropped
    assert {c["a"] for c in mg.CASES.values()} == {0, 1, 2}


# ------------------------------------------------------------------------------------------------ the sweep
def test_sweep_covers_what_it_must():
    cases = list(mg.SWEEP.values())
    for e in range(8):  # every e at its smallest defined length and one above
        assert {c["L"] for c in cases if c["e"] == e and c["a"] == 1} >= {12 * (e + 2) + 13, 12 * (e + 2) + 14}
    assert (mg.min_defined_length(0, 1), mg.min_defined_length(3, 1), mg.min_defined_length(7, 1)) == (37, 73, 121)
    assert {c["a"] for c in cases} == {0, 1, 2} and {c["L"] for c in cases} >= {100, 150, 300, 1000}
    assert max(c["n_reads"] for c in cases) > 10_000  # the reference loads batches of 10 000


@pytest.mark.parametrize("key", sorted(mg.SWEEP))
def test_sweep_case(key):
    case = mg.SWEEP[key]
    e, a, stages = case["e"], case["a"], case.get("stages", True)
    inp = mg.sweep_inputs(case)
    got, res, _, _ = mg.oracle_outcome(inp, e, a, with_result=True)
    comparable(inp, e, a, got)
    assert np.array_equal(got["stats"], recorded("sweep/%s/stats" % key))
    assert np.array_equal(mg.digests(got, stages), recorded("sweep/%s/digests" % key))
    if LIVE:
        live = mg.reference_outcome(inp, e, a, stages=stages)
        same_outcome(live, got, ["stats", "index_sha256"] + mg.RECORD_KEYS + (mg.STAGE_KEYS if stages else []), "live reference vs oracle")
        assert live["sam_text"] == got["sam_text"]
        if stages:
            assert alignments_agree(inp, e, a, res) == int(got["stats"][4])


# ------------------------------------------------------------------------------------------------ the undefined regions
def oracle_asserts(inp, e=3, a=1):
    """uint8[n_reads]: 1 where the oracle marks a record of that read, mapped alone, with 0x8000."""
    ref = fo.Reference(inp.seqs)
    idx = fo.OracleIndex(ref, mg.K, mg.STEP)
    out = np.zeros(len(inp.reads), np.uint8)
    for i, r in enumerate(inp.reads):
        res = fo.map_reads(ref, idx, fo.ReadBatch([r]), e=e, a=a)
        out[i] = bool((res.r_flag & 0x8000).any())
    return out


def test_lower_case_the_reference_aborts_exactly_where_the_oracle_says():
    inp = mg.Inputs.from_arrays({k: recorded(k) for k in ("lower_text", "lower_lens", "lower_bases", "lower_offs")}, "lower_")
    assert 35 <= len(inp.reads) <= 45 and any(s != s.upper() for s in inp.seqs)
    want = recorded("lower_aborts")
    assert 5 < int(want.sum()) < len(want) - 5  # both outcomes occur
    assert np.array_equal(oracle_asserts(inp), want)
    if LIVE:
        assert np.array_equal(mg.lowercase_aborts(inp), want)  # each read alone in a child process: SIGABRT or a clean end


@pytest.mark.parametrize("e", range(8))
@pytest.mark.parametrize("a", [0, 1, 2])
def test_one_seed_short_of_the_table_the_oracle_returns_no_candidates(e, a):
    # G = R lg - 1 in the smallest phase group: the reference reads R uninitialised Seeds there (src/filter.c:5-7, 30-41), so
    # there is nothing of it to compare with; the oracle's choice is no candidates (fem_oracle.c, fo_seed_candidates)
    R, lg = e + 1 + a, (mg.K + mg.STEP - 1) // mg.STEP
    rng = np.random.default_rng(900 + 10 * e + a)
    from tests import util
    seqs = [util.rand_seq(rng, 20_000)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref, mg.K, mg.STEP)
    for L in range(mg.min_defined_length(e, a) - mg.STEP, mg.min_defined_length(e, a)):
        assert (L - mg.K + 1 - (mg.STEP - 1)) // mg.STEP == R * lg - 1  # inside the formula's region
        reads = util.make_reads(rng, seqs, 40, L, 0)  # exact copies: they would map if seeds were chosen
        res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, a=a)
        assert len(res.cands) == 0 and int(res.stats[3]) == 0 and int(res.stats[1]) == 0 and len(res.r_flag) == 0
    reads = util.make_reads(rng, seqs, 40, mg.min_defined_length(e, a), 0)  # one base more: defined, and (R > 1) they map
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, a=a)
    assert (int(res.stats[1]) >= 36) if R > 1 else (int(res.stats[1]) == 0)  # (a few may touch a border of the sequence)
