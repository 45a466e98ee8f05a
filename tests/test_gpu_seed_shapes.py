"""Seed lengths and steps other than 12 / 3 on the device: the index build (hash_entries_kernel and the sort over 2 k bits,
fem_amd/csrc/fem_index_build.hip), the generic seeding kernel (seed_filter_kernel, fem_amd/csrc/fem_kernels.hip.h) on both of
its DP forms and both of its list paths, its shape gate, the fast kernels over an occurrence table whose step is not the
mapping's, packed staging and the tail at another k, and `FEM index K S` / `FEM map` over such files — each against the
oracle, array for array or byte for byte.  k = 16, which has no defined meaning, is refused.

The reference, the reads and the edits are those of tests/test_gpu_verify_packed.py (tests/cases.py).  Needs a GPU: -m gpu."""
import os

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import util
from tests.cases import expected_sam, packed_reads, packed_reference, write_case
from tests.harness import assert_same_records, device_with_env, run_fem, run_packed

pytestmark = pytest.mark.gpu

N_READS = 400

# (k, step) of the index build against the oracle
BUILD_PAIRS = [(12, 1), (12, 2), (12, 4), (12, 12), (11, 4), (13, 5), (14, 3), (7, 16), (10, 16), (5, 7), (1, 1), (2, 1),
               (8, 13), (12, 17)]

# (k, step, L, e, a) of the generic kernel against the oracle
CASES = [
    (12, 1, 100, 3, 1),    # lg = 12
    (12, 2, 100, 3, 1),
    (12, 4, 100, 3, 1),
    (12, 6, 150, 3, 1),
    (12, 12, 150, 3, 1),   # step = k; serial DP: 2 * 12 * 5 > 64
    (11, 4, 100, 3, 1),    # k no multiple of step, lg = 3
    (14, 3, 100, 3, 1),    # (the one case on the 1 GiB lookup table)
    (7, 16, 100, 0, 1),    # 32 phase groups in the DPP form: 2 * 16 * 2 = 64 exactly
    (7, 16, 150, 1, 1),    # serial DP on 32 lanes
    (10, 16, 300, 3, 1),   # step > k, lg = 1
    (5, 7, 100, 3, 2),     # R = 6, long lists
    (8, 13, 100, 1, 0),    # a = 0
    (9, 2, 300, 7, 2),     # 97 DP columns: serial
    (12, 1, 1024, 7, 2),   # 894 columns
    (6, 16, 1024, 7, 2),   # short and long lists in one batch
    (12, 5, 301, 3, 1),    # 44 columns
    (5, 5, 100, 3, 1),     # k <= 6 in the DPP form (2 * 5 * 5 = 50 lanes): long lists behind it
]


def _lg(k, step):
    return -(-k // step)


def _gate_open(L, k, step, e, a):
    """src/filter.c:161-172: a read of L bases is seeded at all."""
    S, R = L - k + 1, e + 1 + a
    return S > 0 and R <= S // step and (S - (step - 1)) // step - R * _lg(k, step) >= 0


def _dpp_form(L, k, step, e, a):
    """seed_filter_kernel: every (strand, phase group, row) in a lane of its own and the columns within 64 lanes."""
    S, R = L - k + 1, e + 1 + a
    return 2 * step * R <= 64 and S // step - R * _lg(k, step) + 1 <= 64


class _World:
    def __init__(self):
        rng = np.random.default_rng(20260117)
        self.seqs, self.places = packed_reference(rng)
        self.ref = fo.Reference(self.seqs)
        self.idx = {}
        self.devs = {}
        self.cases = {}
        self._scratch = None

    def index(self, k, step):
        if (k, step) in self.idx:
            return self.idx[(k, step)]
        idx = fo.OracleIndex(self.ref, k, step, threads=4 if k >= 13 else 1)
        if k < 13:  # (256 MiB and 1 GiB of lookup table are not kept)
            self.idx[(k, step)] = idx
        return idx

    def dev(self, k, step, built=False, force_hash=False):
        """A handle with the reference and its (k, step) index: built on the device or the oracle's, uploaded."""
        key = (k, step, force_hash)
        if key not in self.devs:
            assert os.environ.get("FEM_FORCE_HASH", "0") == "0"
            d = device_with_env(**({"FEM_FORCE_HASH": "1"} if force_hash else {}))
            d.upload_reference(self.seqs)
            if built:
                d.build_index(k, step, fetch=False)
            else:
                idx = self.index(k, step)
                d.upload_index(k, step, idx.lookup, idx.occ[:idx.n_occ])
            self.devs[key] = d
        return self.devs[key]

    def scratch(self):
        """A handle whose reference and index every user replaces."""
        if self._scratch is None:
            from fem_amd import Device
            self._scratch = Device(0)
        return self._scratch

    def case(self, i):
        """(reads, the oracle's seeding and verification) of CASES[i], made once."""
        if i not in self.cases:
            k, step, L, e, a = CASES[i]
            reads = packed_reads(np.random.default_rng(8000 + i), self.seqs, self.places, N_READS, L, e)
            self.cases[i] = (reads, _oracle(self, reads, k, step, e, a))
        return self.cases[i]

    def close(self):
        for d in list(self.devs.values()) + ([self._scratch] if self._scratch else []):
            d.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _oracle(world, reads, k, step, e, a, index_step=None, stages=fo.STAGE_SEED | fo.STAGE_VERIFY):
    idx = world.index(k, index_step or step)
    return fo.map_reads(world.ref, idx, fo.ReadBatch(reads), e=e, a=a, k=k, step=step, threads=4, stages=stages)


def _map(dev, reads, k, step, e, a):
    batch = fo.ReadBatch(reads)
    dev.stage_reads(batch.bases, batch.off)
    dev.map_staged(e=e, a=a, k=k, step=step)
    got = dev.fetch()
    return got.per_strand() + (got.stats,)


def _assert_equal(got, want):
    off, cand, ed, end, stats = got
    assert np.array_equal(off, want.cand_off), "candidates per strand"
    assert np.array_equal(cand, want.cands), "candidates"
    assert np.array_equal(ed, want.v_ed), "edit distances"
    assert np.array_equal(end[ed != 255], want.v_end[want.v_ed != 255]), "end positions of the accepted"
    assert len(stats) == 5 and np.array_equal(stats, want.stats), "counters"


def _assert_mix(want, n):
    strand = np.repeat(np.arange(2 * n) & 1, np.diff(want.cand_off.astype(np.int64)))
    ok = want.v_ed != 255
    assert np.any(ok & (strand == 0)) and np.any(ok & (strand == 1)), "accepted candidates on both strands"
    assert np.any(~ok), "rejected candidates"
    per_read = want.cand_off[2::2].astype(np.int64) - want.cand_off[:-1:2].astype(np.int64)
    assert np.count_nonzero(per_read) > 100, "reads with candidates"


# ---------------------------------------------------------------- a. the index build
def _edge_reference(rng, k, step):
    """About 300 sequences: every length around one and two index entries, 1000 + r for each r mod step, N runs of 1, k - 1,
    k and 2 k + 3 that start and end inside k-mers, lower-case stretches (n among them), one sequence of nothing but T,
    many sequences too short for an entry between the others."""
    seqs = [util.rand_seq(rng, n) for n in [1, max(1, k - 1), k, k + 1, k + step - 1, k + step] + [1000 + r for r in range(step)]]
    seqs.append(b"T" * (3 * k + 2 * step + 5))
    s = bytearray(util.rand_seq(rng, 40 * (k + step) + 200))
    at = k // 2 + 1
    for run in (1, max(1, k - 1), k, 2 * k + 3, 1, step, k + 1):
        s[at:at + run] = b"N" * run
        at += run + k + step + 1 + run % 3
    seqs.append(bytes(s))
    s = util.rand_seq(rng, 900)
    seqs.append(s[:50] + s[50:400].lower() + s[400:500] + b"n" * 5 + s[505:700] + s[700:900].lower())
    seqs.append(util.rand_seq(rng, 300).lower())
    while len(seqs) < 300:
        seqs.append(util.rand_seq(rng, int(rng.integers(1, 2 * k + 2 * step)) if len(seqs) % 3 else int(rng.integers(50, 400))))
    return [seqs[int(i)] for i in rng.permutation(len(seqs))]


def _assert_build(dev, seqs, k, step, idx):
    dev.upload_reference(seqs)
    n, lookup, occ = dev.build_index(k, step)
    assert n == idx.n_occ
    assert np.array_equal(lookup, idx.lookup), "lookup table"
    assert np.array_equal(occ, idx.occ[:n]), "occurrence table"
    lookup2, occ2 = dev.fetch_index(k, n)
    assert np.array_equal(lookup2, lookup) and np.array_equal(occ2, occ), "fetched again"
    return n, lookup


@pytest.mark.parametrize("k,step", BUILD_PAIRS)
def test_index_build_equals_the_oracle(world, k, step):
    n, _ = _assert_build(world.scratch(), world.seqs, k, step, world.index(k, step))
    assert n == sum((len(s) - k) // step + 1 for s in world.seqs)


@pytest.mark.parametrize("k,step", BUILD_PAIRS)
def test_index_build_on_short_odd_and_masked_sequences(world, k, step):
    seqs = _edge_reference(np.random.default_rng(100 * k + step), k, step)
    assert len(seqs) == 300 and (k == 1 or sum(len(s) < k for s in seqs) > 10), "sequences without an entry among the others"
    idx = fo.OracleIndex(fo.Reference(seqs), k, step, threads=4 if k >= 13 else 1)
    n, _ = _assert_build(world.scratch(), seqs, k, step, idx)
    assert n == sum((len(s) - k) // step + 1 for s in seqs if len(s) >= k)


def test_index_build_when_no_sequence_holds_a_seed(world):
    rng = np.random.default_rng(12)
    seqs = [util.rand_seq(rng, 1 + i % 11) for i in range(40)]
    n, lookup = _assert_build(world.scratch(), seqs, 12, 4, fo.OracleIndex(fo.Reference(seqs), 12, 4))
    assert n == 0 and not lookup.any()


# ---------------------------------------------------------------- b. the generic kernel
@pytest.mark.parametrize("i", range(len(CASES)), ids=["-".join(map(str, c)) for c in CASES])
def test_generic_kernel_equals_the_oracle(world, i):
    k, step, L, e, a = CASES[i]
    reads, want = world.case(i)
    _assert_mix(want, N_READS)
    dev = world.dev(k, step, built=i % 2 == 1)
    assert dev.seed_kernel(e, a, k, step) == "seed_filter_kernel"
    _assert_equal(_map(dev, reads, k, step, e, a), want)


def test_the_cases_cover_both_dp_forms_and_both_list_paths(world):
    forms = {_dpp_form(L, k, step, e, a) for k, step, L, e, a in CASES}
    assert forms == {True, False}
    assert all(_gate_open(L, k, step, e, a) for k, step, L, e, a in CASES)
    small = large = 0
    both_in_one = False
    for i, (k, step, L, e, a) in enumerate(CASES):
        if k >= 13:
            continue  # (its index is not kept on the host)
        reads, _ = world.case(i)
        idx = world.index(k, step)
        pre = np.array([fo.seed_candidates(world.ref, idx, s, e=e, a=a, k=k, step=step)[1]
                        for r in reads[:60] for s in (r, fo.revcomp(r))])
        pre = pre[pre > 0]
        small += int(np.count_nonzero(pre <= 64))
        large += int(np.count_nonzero(pre > 64))
        both_in_one |= bool(np.any(pre <= 64) and np.any(pre > 64))
    # strands whose selected occurrences fit the lanes of one wave (strand_small) and strands that take the list path
    assert small > 0 and large > 0 and both_in_one


# ---------------------------------------------------------------- c. the shape gate
def test_the_shape_gate_at_13_5_closes_at_150_bases_and_opens_at_151(world):
    k, step, e, a = 13, 5, 7, 1
    assert not _gate_open(150, k, step, e, a) and _gate_open(151, k, step, e, a)
    dev = world.dev(k, step, built=True)
    assert dev.seed_kernel(e, a, k, step) == "seed_filter_kernel"
    for L in (150, 151):
        reads = packed_reads(np.random.default_rng(7100 + L), world.seqs, world.places, N_READS, L, e)
        want = _oracle(world, reads, k, step, e, a)
        got = _map(dev, reads, k, step, e, a)
        _assert_equal(got, want)
        if L == 150:
            assert len(got[1]) == 0 and not got[0].any() and int(got[4][0]) == N_READS and not got[4][1:].any()
        else:
            _assert_mix(want, N_READS)


def test_a_batch_of_reads_on_both_sides_of_the_gate(world):
    k, step, e, a = 11, 4, 3, 1
    gate = next(L for L in range(k, 300) if _gate_open(L, k, step, e, a))
    assert gate == 73 and not any(_gate_open(L, k, step, e, a) for L in range(gate))
    rng = np.random.default_rng(7200)
    lengths = [k - 1, k, gate - 1, gate, 100, 257]  # (the layout is sized from the longest)
    reads = []
    for L in lengths:
        reads += packed_reads(rng, world.seqs, world.places, 67, L, e)
    reads = [reads[int(j)] for j in rng.permutation(len(reads))]
    want = _oracle(world, reads, k, step, e, a)
    dev = world.dev(k, step)
    got = _map(dev, reads, k, step, e, a)
    _assert_equal(got, want)
    per_read = got[0][2::2].astype(np.int64) - got[0][:-1:2].astype(np.int64)
    below = np.array([len(r) < gate for r in reads])
    assert not per_read[below].any(), "reads under the gate come back with empty ranges"
    for L in lengths[3:]:
        assert per_read[np.array([len(r) == L for r in reads])].any(), L


# ---------------------------------------------------------------- d. an index whose step is not the mapping's
@pytest.mark.parametrize("s,force_hash", [(1, False), (2, False), (4, False), (6, False), (17, False), (1, True)])
def test_mapping_at_12_3_over_an_index_of_another_step(world, s, force_hash):
    L, e = 100, 3
    reads = packed_reads(np.random.default_rng(7300), world.seqs, world.places, N_READS, L, e)
    want = _oracle(world, reads, 12, 3, e, 1, index_step=s)
    base = _oracle(world, reads, 12, 3, e, 1)
    assert int(want.stats[3]) != int(base.stats[3]) and int(want.stats[4]) != int(base.stats[4]), "the step shows"
    dev = world.dev(12, s, built=s in (2, 6), force_hash=force_hash)
    assert "dense" not in dev.index_info()
    assert dev.seed_kernel(e, 1, 12, 3) == ("seed_fast_kernel<hash>" if force_hash else "seed_fast_kernel<lean>")
    _assert_equal(_map(dev, reads, 12, 3, e, 1), want)


def test_map_staged_refuses_a_step_of_17_and_another_k(world):
    from fem_amd import FemError
    dev = world.dev(12, 17)
    reads = packed_reads(np.random.default_rng(7300), world.seqs, world.places, 8, 100, 3)
    batch = fo.ReadBatch(reads)
    dev.stage_reads(batch.bases, batch.off)
    with pytest.raises(FemError, match="out of range"):
        dev.map_staged(e=3, a=1, k=12, step=17)
    with pytest.raises(FemError, match="differs"):
        dev.map_staged(e=3, a=1, k=8, step=3)


# ---------------------------------------------------------------- e. packed staging and the tail at another k
@pytest.mark.parametrize("i", [CASES.index((11, 4, 100, 3, 1)), CASES.index((7, 16, 150, 1, 1))])
def test_packed_staging_and_records_at_another_k(world, i):
    k, step, L, e, a = CASES[i]
    reads, want = world.case(i)
    dev = world.dev(k, step, built=i % 2 == 1)
    off, cand, ed, end, stats = run_packed(dev, reads, L, e, k, step)
    _assert_equal((off, cand, ed, end, stats), want)
    rec = dev.fetch_records()
    full = _oracle(world, reads, k, step, e, a, stages=fo.STAGE_SEED | fo.STAGE_VERIFY | fo.STAGE_ALIGN)
    assert int(full.stats[4]) > 100
    assert_same_records(full, rec)


# ---------------------------------------------------------------- f. the command line
@pytest.mark.parametrize("k,step,batch", [(8, 4, None), (11, 4, None), (12, 1, "97"), (12, 6, None)])
def test_cli_index_files_of_other_shapes_and_map_over_them(tmp_path, k, step, batch):
    e = 3
    seqs, names, reads, rnames, quals, fa, fq = write_case(tmp_path, 300 + 10 * k + step, e, 100, 600, False)
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref, k, step)
    index_path, oracle_index, sam_path = str(tmp_path / "ref.idx"), str(tmp_path / "o.idx"), str(tmp_path / "out.sam")
    r = run_fem("index", str(k), str(step), fa, index_path)
    assert r.returncode == 0, r.stderr.decode()
    idx.save(oracle_index)
    assert open(index_path, "rb").read() == open(oracle_index, "rb").read()
    if k == 11:
        return
    r = run_fem("map", "-e", str(e), "-t", "3", "--ref", fa, "--index", index_path, "--read1", fq, "-o", sam_path,
            *(["--batch", batch] if batch else []))
    if k != 12:
        assert r.returncode != 0 and b"Index was built with k=8" in r.stderr
        return
    assert r.returncode == 0, r.stderr.decode()
    want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, k=12, step=3)  # FEM map: k = 12, step = 3 whatever the file says
    assert int(want.stats[4]) > 300
    text = open(sam_path).read()
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(names, seqs))
    assert text.startswith(header)
    assert text[len(header):] == expected_sam(names, reads, rnames, quals, want)
    err = r.stderr.decode()
    for label, v in zip(["The number of read", "The number of mapped read",
                         "The number of candidate before additional q-gram filter", "The number of candidate",
                         "The number of mapping"], want.stats):
        assert "%s: %d\n" % (label, int(v)) in err


# ---------------------------------------------------------------- k = 16 and k = 0 are refused
def test_the_device_refuses_a_seed_length_of_16_and_of_0(world):
    from fem_amd import FemError
    dev = world.scratch()
    dev.upload_reference(world.seqs[:1])
    for k in (16, 0):
        with pytest.raises(FemError, match=r"k must be 1\.\.15 and step >= 1"):
            dev.upload_index(k, 3, np.zeros(5, np.uint32), np.zeros(1, np.uint64), n_occ=0)
        with pytest.raises(FemError, match=r"k must be 1\.\.15 and step >= 1"):
            dev.build_index(k, 3, fetch=False)
    dev = world.dev(12, 4)
    batch = fo.ReadBatch(packed_reads(np.random.default_rng(1), world.seqs, world.places, 4, 100, 3))
    dev.stage_reads(batch.bases, batch.off)
    with pytest.raises(FemError, match=r"out of range \(k 1\.\.15"):
        dev.map_staged(e=3, a=1, k=16, step=4)
