"""Reads of 256..1024 bases (kMaxReadLen, the device path's limit) through every device path, against the CPU oracle and
the models of tests/: the seed kernels (lean fast form and its hand-off to the generic kernel, the hash-join form, the
dense selection with its take masks of one, two and four words and its hand-off above 128 columns, banks), verification,
the tail with MD strings beyond the first pass's staging, the SAM kernels, the packed transfer, read pairs with mates that
overlap, contain one another and dovetail, the limits of the C ABI and `FEM map` end to end.  Each case asserts that its
fixture reaches the path it is named for.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import pair_model as pm
from tests import util
from tests.cases import banked_reference, expected_sam, make_pairs
from tests.harness import assert_same, assert_same_records, banked_compare, banked_device, build_index, dense_setup
from tests.harness import device_with_env, fetch_sam, open_reference, run_fem

pytestmark = pytest.mark.gpu

MAX_LEN = 1024
THREADS = 16
BLOCK = 16            # reads per block of seed_fast_kernel (femk::kReadBlock)
LEAN_CHARS = 16 * 256  # a block of the lean form holds at most this many characters when the batch has a read over 256
MD_CAP = 32           # first-pass MD staging per record of the tail (fem_tail.hip: kMdCap)
ODD = b"RYKM=.-*"     # characters outside ACGTN, as test_gpu_sam.py uses them


def widest(L, R):
    """Columns of phase group 0 in the seed selection DP (fem_seed_select.hip.h: S / step - R * lg + 1)."""
    return (L - 11) // 3 - 4 * R + 1


def _damage(rng, reads, lower_every=9, odd_every=7, n_run_every=11):
    """Lower-case reads, IUPAC / punctuation characters and N runs in some of the reads."""
    out = []
    for i, r in enumerate(reads):
        if i % lower_every == 4:
            r = r.lower()
        elif i % odd_every == 3:
            at = int(rng.integers(0, len(r) - len(ODD)))
            r = r[:at] + ODD[:1 + i % len(ODD)] + r[at + 1 + i % len(ODD):]
        elif i % n_run_every == 5:
            at = int(rng.integers(0, len(r) - 6))
            r = r[:at] + b"N" * 5 + r[at + 5:]
        out.append(r)
    return out


def _sam_fields(text):
    """SAM lines split into fields, SEQ (which goes through the 4-bit BAM round trip) aside."""
    return [l.split("\t")[:9] + l.split("\t")[10:] for l in text.splitlines()]


# ---------------------------------------------------------------------------------------------------------------------
# a. sparse index: seed_fast_kernel<lean> and the generic kernel, the tail, the SAM text; default and tiny staging
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse():
    from fem_amd import host
    rng = np.random.default_rng(1024)
    # a random reference of a few Mbp, one sequence shorter than the longest reads and one of 13 bases
    seqs = [util.rand_seq(rng, 3_000_000), util.rand_seq(rng, 2_000_000), util.rand_seq(rng, 1000), util.rand_seq(rng, 13)]
    names = ["chr%d_%s" % (i, "x" * (40 * i)) for i in range(len(seqs))]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref, threads=THREADS)
    devs = {"default": device_with_env(FEM_TEST_TINY_BUFFERS=0), "tiny-staging": device_with_env(FEM_TEST_TINY_BUFFERS=1)}
    for d in devs.values():
        d.upload_reference(seqs)
        d.upload_reference_names(names)
        d.upload_index(12, 3, idx.lookup, idx.occ[:idx.n_occ])
    tref = host.TailReference(ref.text, ref.off, ref.len, names=names)
    yield dict(rng=rng, seqs=seqs, names=names, ref=ref, idx=idx, devs=devs, tref=tref)
    for d in devs.values():
        d.close()


def _without_reads(text, skip):
    return [l for l in text.splitlines() if l.split("\t", 1)[0] not in skip]


def _full_compare(s, reads, e, a, slot=0):
    """Every output of the batch on both devices against the oracle: candidates (fetch, fetch_packed), records, SAM text."""
    from fem_amd import host
    batch = fo.ReadBatch(reads)
    want = fo.map_reads(s["ref"], s["idx"], batch, e=e, a=a, threads=THREADS)
    rnames = ["long_%d_%s" % (i, "n" * (i % 90)) for i in range(len(reads))]
    quals = ["".join(chr(33 + (13 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
    q = np.frombuffer("".join(quals).encode(), np.uint8)
    for name, dev in s["devs"].items():
        dev.stage_reads(batch.bases, batch.off, slot=slot)
        dev.stage_text(q, rnames, slot=slot)
        dev.map_staged(e=e, a=a, slot=slot)
        assert_same(want, dev.fetch(slot=slot))
        assert_same(want, dev.fetch_packed(slot=slot))
        rec = dev.fetch_records(slot=slot)
        assert_same_records(want, rec)
        text, n_records, n_asserted, stats = dev.fetch_sam(slot=slot)
        assert np.array_equal(stats, want.stats) and n_records == int(want.rec_off[-1]), name
        host_text, host_asserted = host.records_sam(s["tref"], rnames, batch.bases, batch.off, q, rec, threads=4, parts=True)
        assert text.decode("latin-1") == host_text and n_asserted == host_asserted, name
        # ... and with the text built from the oracle's records, on the reads none of whose records the reference would have
        # asserted on (those are written with CIGAR '*', which expected_sam does not model)
        ro = want.rec_off.astype(np.int64)
        skip = {rnames[r] for r in range(len(reads)) if np.any(want.r_flag[ro[r]:ro[r + 1]] & 0x8000)}
        got_lines = _sam_fields("\n".join(_without_reads(text.decode("latin-1"), skip)))
        want_lines = _sam_fields("\n".join(_without_reads(expected_sam(s["names"], reads, rnames, quals, want), skip)))
        assert got_lines == want_lines, name
        assert len(want_lines) > 0.9 * int(want.rec_off[-1]), "the comparison with expected_sam must cover the batch's records"
    return want


def _deletion_reads(rng, seqs, n, L, k):
    """Reads with k single-base deletions ~L/(k+1) apart: MD strings of k + 1 numbers and k '^X' runs, beyond MD_CAP."""
    out = []
    for _ in range(n):
        at = int(rng.integers(0, len(seqs[0]) - L - k - 1))
        w = bytearray(seqs[0][at:at + L + k])
        for j in range(k, 0, -1):
            del w[j * L // (k + 1)]
        out.append(bytes(w) if rng.random() < 0.5 else util.revcomp(bytes(w)))
    return out


def _assert_long_md(want):
    md_len = np.diff(want.md_off.astype(np.int64))
    assert (md_len > MD_CAP).sum() > 0, "fixture must hold MD strings beyond the first pass's staging"


@pytest.mark.parametrize("e,a,L,n", [(0, 1, 256, 120), (3, 1, 257, 120), (5, 2, 300, 100), (7, 1, 301, 100), (3, 0, 443, 80),
                                     (7, 2, 515, 80), (5, 1, 700, 60), (3, 2, 1000, 50), (7, 1, 1023, 50), (7, 2, 1024, 50)])
def test_uniform_long_batches_on_a_sparse_index(sparse, e, a, L, n):
    s = sparse
    assert s["devs"]["default"].seed_kernel(e=e, a=a) == "seed_fast_kernel<lean>"
    rng = np.random.default_rng(3100 + 10 * e + a + L)
    # (on a sparse index the seeds of a read with edits often fall on 12-mers the index does not hold: few of those map)
    reads = util.make_reads(rng, s["seqs"], n // 2, L, e + 1) + util.make_reads(rng, s["seqs"], n - n // 2, L, 0)
    reads = _damage(rng, reads)
    assert len(set(map(len, reads))) == 1
    # every full block of 16 reads goes to the generic kernel except at L = 256, where 16 * 256 characters just fit the lean
    # kernel's staging (a last, partial block of a batch may fit it at any length)
    assert (L * BLOCK <= LEAN_CHARS) == (L == 256), "full blocks of these reads go to the generic kernel, save at 256 bases"
    want = _full_compare(s, reads, e, a, slot=L % 4)
    assert want.stats[1] > n // 2


def _mixed_blocks(rng, seqs, e, blocks):
    """Reads in blocks of 16: a block is (long read lengths, short read length); the long reads at random places in it."""
    reads = []
    for longs, short in blocks:
        blk = [util.make_reads(rng, seqs, 1, L, e)[0] for L in longs]
        blk += util.make_reads(rng, seqs, BLOCK - len(longs), short, e)
        reads += [blk[i] for i in rng.permutation(BLOCK)]
    return reads


@pytest.mark.parametrize("e,a", [(3, 1), (7, 1), (5, 2), (0, 1)])
def test_mixed_blocks_split_between_the_lean_kernel_and_the_generic_kernel(sparse, e, a):
    # seed_fast_kernel<lean> stages a block of 16 reads when its characters fit 16 * min(max_len, 256): one 1000-base read
    # among fifteen of 100 bases stays in the lean kernel; three of them (or sixteen of 300) go to the generic kernel
    s = sparse
    rng = np.random.default_rng(3200 + 10 * e + a)
    blocks = [((1000,), 100), ((1024,), 190), ((300, 257), 150), ((700,), 100), ((1000, 1000, 1000), 100), ((), 300),
              ((1023, 515), 120), ((), 100), ((443,), 200), ((1024, 1024, 1024, 1024), 90), ((256,), 100), ((301,), 230)] * 2
    reads = _damage(rng, _mixed_blocks(rng, s["seqs"], e, blocks))
    lens = np.array([len(r) for r in reads])
    assert lens.max() > 256
    totals = lens.reshape(-1, BLOCK).sum(axis=1)
    longest = lens.reshape(-1, BLOCK).max(axis=1)
    assert np.any((longest > 256) & (totals <= LEAN_CHARS)), "fixture must hold blocks with a long read in the lean kernel"
    assert np.any(totals > LEAN_CHARS), "fixture must hold blocks for the generic kernel"
    want = _full_compare(s, reads, e, a, slot=1)
    assert want.stats[1] > len(reads) // 5


def test_long_reads_at_the_ends_of_sequences_and_in_the_short_ones(sparse):
    # reads over both ends of every sequence (range clip), reads longer than the 1000-base sequence, around the 13-base one
    s = sparse
    rng = np.random.default_rng(3300)
    reads = []
    for sq in s["seqs"][:3]:
        for L in (300, 1000, 1024):
            for at in (0, 1, 3, 7):
                r = sq[at:at + L]
                if len(r) == L:
                    reads += [r, util.revcomp(r)]
            for back in (0, 2, 9):
                r = sq[len(sq) - L - back:len(sq) - back] if len(sq) >= L + back else b""
                if len(r) == L:
                    reads += [r, util.revcomp(r)]
    reads += [s["seqs"][2] + util.rand_seq(rng, 24), util.rand_seq(rng, 11) + s["seqs"][2][:1013], s["seqs"][3] * 40]
    reads += util.make_reads(rng, s["seqs"], 40, 800, 3)
    want = _full_compare(s, reads, 3, 1, slot=2)
    assert want.stats[1] > 40


# ---------------------------------------------------------------------------------------------------------------------
# e. packed transfer of uniform long batches: commit_stage_packed, stage_reads and the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,e", [(257, 3), (512, 5), (1021, 7), (1024, 3)])
def test_packed_long_reads_three_ways(sparse, L, e):
    from fem_amd import device
    s = sparse
    dev = s["devs"]["default"]
    rng = np.random.default_rng(3400 + L)
    n = 96
    reads = util.make_reads(rng, s["seqs"], n, L, e)
    reads[0] = b"N" + reads[0][1:]
    reads[-1] = reads[-1][:-1] + b"n"
    reads[5] = reads[5].lower()
    for i in range(7, n, 9):
        at = int(rng.integers(0, L - 4))
        reads[i] = reads[i][:at] + b"NNNN" + reads[i][at + 4:]
    batch = fo.ReadBatch(reads)
    want = fo.map_reads(s["ref"], s["idx"], batch, e=e, threads=THREADS)
    hb, _ = dev.acquire_stage(n, n * L, slot=3)
    n_exc = device.pack_reads(batch.bases, n, L, hb)
    assert n_exc == sum(sum(1 for c in r if c not in b"ACGT") for r in reads) and n_exc > L
    dev.commit_stage_packed(n, L, n_exc, slot=3)
    assert dev.stage_info(3)[1]
    dev.map_staged(e=e, slot=3)
    assert_same(want, dev.fetch(slot=3))
    assert_same_records(want, dev.fetch_records(slot=3))
    dev.stage_reads(batch.bases, batch.off, slot=2)
    assert dev.stage_info(2)[1], "a uniform batch with few exceptions crosses the link packed"
    dev.map_staged(e=e, slot=2)
    assert_same(want, dev.fetch(slot=2))
    assert_same_records(want, dev.fetch_records(slot=2))
    assert want.stats[1] > n // 4


# ---------------------------------------------------------------------------------------------------------------------
# g. the limits at the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_the_abi_takes_1024_and_refuses_1025(sparse):
    from fem_amd import FemError, device
    s = sparse
    dev = s["devs"]["default"]
    assert dev.limits()[0] == MAX_LEN
    rng = np.random.default_rng(3500)
    reads = util.make_reads(rng, s["seqs"], 40, MAX_LEN, 3)
    too_long = util.make_reads(rng, s["seqs"], 1, MAX_LEN + 1, 3)[0]
    bad = fo.ReadBatch(reads[:20] + [too_long] + reads[20:])
    with pytest.raises(FemError, match="1024"):
        dev.stage_reads(bad.bases, bad.off, slot=0)
    n = len(bad.off) - 1
    hb, ho = dev.acquire_stage(n, len(bad.bases), slot=0)
    hb[:len(bad.bases)] = bad.bases
    ho[:n + 1] = bad.off
    with pytest.raises(FemError, match="1024"):
        dev.commit_stage(n, MAX_LEN + 1, slot=0)
    hb, _ = dev.acquire_stage(8, 8 * (MAX_LEN + 1), slot=0)
    hb[:] = ord("A")
    with pytest.raises(FemError, match="1024"):
        dev.commit_stage(8, MAX_LEN + 1, slot=0, uniform=True)
    with pytest.raises(FemError, match="1024"):
        dev.commit_stage_packed(8, MAX_LEN + 1, 0, slot=0)
    with pytest.raises(FemError):
        dev.reserve_batch(100, 200, MAX_LEN + 1, slot=0)
    dev.reserve_batch(100, 200, MAX_LEN, e=3, slot=0)
    # the handle still maps, and a batch of 1024-base reads comes out the same however it is staged
    good = fo.ReadBatch(reads)
    want = fo.map_reads(s["ref"], s["idx"], good, e=3, threads=THREADS)
    n = len(reads)

    def check(slot):
        dev.map_staged(e=3, slot=slot)
        assert_same(want, dev.fetch(slot=slot))
        assert_same_records(want, dev.fetch_records(slot=slot))

    dev.stage_reads(good.bases, good.off, slot=0)
    check(0)
    hb, ho = dev.acquire_stage(n, n * MAX_LEN, slot=1)
    hb[:n * MAX_LEN] = good.bases[:n * MAX_LEN]
    ho[:n + 1] = good.off
    dev.commit_stage(n, MAX_LEN, slot=1)
    check(1)
    dev.commit_stage(n, MAX_LEN, slot=1, uniform=True)
    check(1)
    hb, _ = dev.acquire_stage(n, n * MAX_LEN, slot=2)
    n_exc = device.pack_reads(good.bases, n, MAX_LEN, hb)
    dev.commit_stage_packed(n, MAX_LEN, n_exc, slot=2)
    check(2)
    assert want.stats[1] > 15


# ---------------------------------------------------------------------------------------------------------------------
# b / c. the seed kernels the library picks on dense (3 x 72 Mbp) and mid-size (3 x 25 Mbp) indexes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    d = dense_setup(72, [72_000_000] * 3)
    yield d
    d["dev"].close()


@pytest.fixture(scope="module")
def mid():
    d = dense_setup(71, [25_000_000] * 3)
    yield d
    d["dev"].close()


def _edge_long_reads(d, L):
    """Reads at the very start and end of every sequence: the remapped near-start entries (pos < 1024) of the 32-bit table,
    sequences 2048 apart in the global coordinate, the range clip; forward and reverse."""
    out = []
    for o, l in zip(d["off"], d["lens"]):
        sq = d["text"][int(o):int(o) + int(l)]
        for at in (0, 1, 3, 17, 511, 1000, 1023, 1024, 1030):
            r = sq[at:at + L].tobytes()
            out += [r, util.revcomp(r)]
        for back in (0, 2, 9, 1000, 1030):
            r = sq[int(l) - L - back:int(l) - back].tobytes()
            out += [r, util.revcomp(r)]
    return out


def _synth(d, seed, n, L, e):
    from fem_amd import host
    bases, offsets = host.synth_reads(seed, d["text"], d["off"], d["lens"], n, L, e, threads=8)
    return [bases[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(n)]


def _dev_compare(d, reads, e, a, records):
    batch = fo.ReadBatch(reads)
    stages = fo.STAGE_SEED | fo.STAGE_VERIFY | (fo.STAGE_ALIGN if records else 0)
    want = fo.map_reads(d["ref"], d["idx"], batch, e=e, a=a, threads=THREADS, stages=stages)
    dev = d["dev"]
    dev.stage_reads(batch.bases, batch.off, slot=1)
    dev.map_staged(e=e, a=a, slot=1)
    assert_same(want, dev.fetch(slot=1))
    if records:
        assert_same_records(want, dev.fetch_records(slot=1))
    return want


@pytest.mark.parametrize("e,a,lengths", [
    (2, 1, (152, 155, 248, 251, 440, 443, 1000)),   # R = 4:  widest 32 / 33, 64 / 65, 128 / 129, 314
    (7, 2, (224, 227, 320, 323, 512, 515, 1024)),   # R = 10: widest 32 / 33, 64 / 65, 128 / 129, 298
])
def test_dense_selection_take_masks_and_hand_off(dense, e, a, lengths):
    d = dense
    assert d["dev"].seed_kernel(e=e, a=a) == "seed_join_kernel"
    R = e + 1 + a
    w = sorted({widest(L, R) for L in lengths})
    for lo, hi in ((32, 33), (64, 65), (128, 129)):
        assert lo in w and hi in w, "fixture must reach both sides of %d columns" % lo
    assert max(w) > 128, "fixture must hold reads the selection kernel hands to the generic kernel"
    rng = np.random.default_rng(3600 + R)
    reads = []
    for i, L in enumerate(lengths):
        reads += _synth(d, 3600 + 10 * R + i, 70 if L < 900 else 40, L, e)
    reads = [reads[i] for i in rng.permutation(len(reads))]  # mixed lengths inside blocks
    reads += _edge_long_reads(d, 1000) + _edge_long_reads(d, 1024)
    reads = _damage(rng, reads, lower_every=23, odd_every=29, n_run_every=31)
    if e == 7:  # seven deletions in a 1024-base read: MD strings beyond the first pass's staging (default buffers)
        reads += _deletion_reads(rng, [d["text"][int(d["off"][0]):int(d["off"][0]) + int(d["lens"][0])]], 80, 1024, 7)
    want = _dev_compare(d, reads, e, a, records=True)
    if e == 7:
        _assert_long_md(want)
    assert want.stats[1] > 0.7 * len(reads)
    lens = np.array([len(r) for r in reads])
    assert lens.max() == 1024 and lens.min() == min(lengths)


@pytest.mark.parametrize("e,a,L,n", [(3, 1, 400, 200), (7, 1, 1024, 80)])
def test_hash_join_form_on_long_reads(mid, e, a, L, n):
    d = mid
    assert d["dev"].seed_kernel(e=e, a=a) == "seed_fast_kernel<hash>"
    reads = _synth(d, 3700 + L, n, L, e) + _edge_long_reads(d, L)
    want = _dev_compare(d, reads, e, a, records=L == 1024)
    assert want.stats[1] > 0.4 * len(reads)


# ---------------------------------------------------------------------------------------------------------------------
# d. a reference in banks
# ---------------------------------------------------------------------------------------------------------------------
def test_banked_reference_with_long_reads():
    rng = np.random.default_rng(3800)
    seqs = banked_reference(rng, 7, shared=True)
    L, e = 800, 3
    reads = util.make_reads(rng, seqs, 200, L, e, n_rate=0.002)
    for s in seqs:
        reads += [s[:L], s[-L:], fo.revcomp(s[:L]), fo.revcomp(s[-L:]), s[3:3 + L], s[-L - 5:-5]]
    dev = banked_device(110_000)
    try:
        want = banked_compare(dev, seqs, reads, e, 1)
        assert want.stats[1] > len(reads) // 4
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# f. read pairs with long mates
# ---------------------------------------------------------------------------------------------------------------------
def _placed_pairs(rng, seqs, n, L1, L2, e, max_edits=1):
    """Pairs placed by mate start: mate 1 forward at p, mate 2 reverse at p + d, d over a range in which the mates overlap,
    one contains the other, they dovetail (mate 2 starting first) or lie up to ~2 kbp apart; mates swapped half the time."""
    lens = np.array([len(s) for s in seqs], np.int64)
    ok = np.nonzero(lens > 6000)[0]

    def mut(s, ln):
        s = util.mutate(rng, s, int(rng.integers(0, max_edits + 1)))[:ln]
        return s + util.rand_seq(rng, ln - len(s)) if len(s) < ln else s

    r1, r2 = [], []
    for i in range(n):
        si = int(ok[rng.integers(0, len(ok))])
        d = int(rng.integers(-300, 2100))
        p = int(rng.integers(400, lens[si] - 3500))
        a = mut(seqs[si][p:p + L1 + e], L1)
        b = mut(util.revcomp(seqs[si][p + d:p + d + L2 + e])[e:], L2) if i % 17 else util.rand_seq(rng, L2)
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    return r1, r2


@pytest.mark.parametrize("L1,L2,n,X", [(250, 250, 300, 800), (300, 300, 300, 2000), (600, 1024, 160, 2000)])
def test_long_mates_equal_the_pair_model(L1, L2, n, X):
    rng, dev, ref, idx, seqs, names = open_reference(3900 + L1, False, 50_000, 7)
    try:
        e = 3
        if L2 <= 300:
            r1, r2 = make_pairs(rng, seqs, n // 3, L1, e, L2)
            p1, p2 = _placed_pairs(rng, seqs, n - n // 3, L1, L2, e)
            r1, r2 = r1 + p1, r2 + p2
        else:
            r1, r2 = _placed_pairs(rng, seqs, n, L1, L2, e)
        r1[3] = r1[3].lower()
        r2[5] = r2[5][:L2 // 2] + ODD + r2[5][L2 // 2 + len(ODD):]
        reads = r1 + r2
        base = ["lp%d_%s" % (i, "n" * (i % 60)) for i in range(n)]
        rnames = base + base
        quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
        want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=THREADS)
        dev.set_pairs(0, X, slot=1)
        text, n_records, _, stats = fetch_sam(dev, reads, rnames, quals, e, slot=1)
        assert np.array_equal(stats, want.stats) and n_records == int(want.rec_off[-1])
        exp = pm.sam_lines(want, n, names, reads, rnames, quals, 0, X)
        assert _sam_fields(text.decode("latin-1")) == _sam_fields(exp)
        lines, n_proper = pm.expected(want, n, 0, X)
        assert dev.pair_count(slot=1) == n_proper
        got = dev.fetch_pairs(slot=1)
        for k, v in pm.pair_arrays(want, n, 0, X).items():
            if k == "n_proper":
                assert got.n_proper == v
            else:
                assert np.array_equal(getattr(got, k), v), k
        # the layouts the fixture must hold, from the oracle's primary records of both mates
        ro = want.rec_off.astype(np.int64)
        fwd_first = overlap = contain = dovetail = 0
        for i in range(n):
            j1, j2 = ro[i], ro[n + i]
            if ro[i + 1] - j1 != 1 or ro[n + i + 1] - j2 != 1 or want.r_tid[j1] != want.r_tid[j2]:
                continue
            if not (int(want.r_flag[j1]) ^ int(want.r_flag[j2])) & 16:
                continue
            f, r = (j2, j1) if int(want.r_flag[j1]) & 16 else (j1, j2)
            fs, fe = int(want.r_pos[f]), int(want.r_pos[f]) + pm.span(want, f)
            rs, re_ = int(want.r_pos[r]), int(want.r_pos[r]) + pm.span(want, r)
            fwd_first += fs <= rs
            overlap += fs < rs < fe < re_
            contain += (fs <= rs and re_ <= fe) or (rs <= fs and fe <= re_)
            dovetail += rs < fs
        assert overlap > 5 and dovetail > 5 and fwd_first > n // 4, (overlap, dovetail, fwd_first)
        assert contain > 5 or L1 == L2, "fixture must hold mates that contain one another"  # (equal lengths: rarely exact)
        assert n_proper > n // 6
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# h. FEM map end to end
# ---------------------------------------------------------------------------------------------------------------------
def _write_fastq(path, names, reads, quals):
    path.write_bytes(b"".join(b"@%s c\n%s\n+\n%s\n" % (n.encode(), r, q.encode()) for n, r, q in zip(names, reads, quals)))


@pytest.fixture(scope="module")
def cli_ref(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("long_cli")
    rng = np.random.default_rng(4000)
    seqs = [util.rand_seq(rng, 400_000), util.rand_seq(rng, 150_000)]
    fa = tmp / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    ix = tmp / "ref.idx"
    build_index(fa, ix)
    ref = fo.Reference(seqs)
    return dict(rng=rng, seqs=seqs, fa=fa, ix=ix, ref=ref, idx=fo.OracleIndex(ref))


def _fem_map(c, fq, out, *extra, read2=None, env=None):
    args = ["map", "-e", "3", "-t", "4", "--ref", c["fa"], "--index", c["ix"], "--read1", fq, "-o", out]
    if read2:
        args += ["--read2", read2, "-X", "2000"]
    return run_fem(*args, *extra, env=env, text=True)


def _batch_forms(stderr):
    """How each batch's bases crossed the link, from the per-batch stamps of FEM_STAGE_TIMES=2."""
    return [l.rsplit("bases sent as ", 1)[1] for l in stderr.splitlines() if l.startswith("[FEM] batch ")]


def _counters(stderr):
    return [l for l in stderr.splitlines() if l.startswith("The number of")]


def _want_counters(st):
    return ["The number of read: %d" % st[0], "The number of mapped read: %d" % st[1],
            "The number of candidate before additional q-gram filter: %d" % st[2], "The number of candidate: %d" % st[3],
            "The number of mapping: %d" % st[4]]


@pytest.mark.parametrize("kind", ["uniform-1024", "mixed-150-1024"])
def test_fem_map_long_reads_end_to_end(cli_ref, tmp_path, kind):
    c = cli_ref
    rng = np.random.default_rng(4100 + len(kind))
    if kind == "uniform-1024":  # one length: the packed path
        reads = util.make_reads(rng, c["seqs"], 400, MAX_LEN, 3)
    else:  # lengths 150..1024: the character path
        reads = [util.make_reads(rng, c["seqs"], 1, int(L), 3)[0] for L in rng.integers(150, MAX_LEN + 1, 400)]
        reads[0] = util.make_reads(rng, c["seqs"], 1, MAX_LEN, 3)[0]
    reads = [r[:100] + b"N" + r[101:] if i % 13 == 0 else r for i, r in enumerate(reads)]
    names = ["r%d" % i for i in range(len(reads))]
    quals = ["".join(chr(33 + (7 * i + j) % 41) for j in range(len(r))) for i, r in enumerate(reads)]
    fq = tmp_path / "reads.fq"
    _write_fastq(fq, names, reads, quals)
    want = fo.map_reads(c["ref"], c["idx"], fo.ReadBatch(reads), e=3, threads=THREADS)
    header = "".join("@SQ\tSN:s%d\tLN:%d\n" % (i, len(s)) for i, s in enumerate(c["seqs"]))
    out = tmp_path / "out.sam"
    r = _fem_map(c, fq, out, "--batch", "150", env={"FEM_STAGE_TIMES": "2"})
    assert r.returncode == 0, r.stderr
    assert out.read_text(encoding="latin-1") == header + expected_sam(["s0", "s1"], reads, names, quals, want)
    assert _counters(r.stderr) == _want_counters(want.stats)
    assert want.stats[1] > 150
    form = "2-bit codes" if kind == "uniform-1024" else "characters"
    forms = _batch_forms(r.stderr)
    assert len(forms) >= 3 and set(forms) == {form}, "fixture must take the %s path in every batch" % form


def test_fem_map_long_pairs_end_to_end(cli_ref, tmp_path):
    c = cli_ref
    n = 300
    r1, r2 = _placed_pairs(c["rng"], c["seqs"], n, 300, 300, 3)
    names = ["pair%d" % i for i in range(n)]
    q1 = ["".join(chr(33 + (7 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r1)]
    q2 = ["".join(chr(34 + (5 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r2)]
    p1, p2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    _write_fastq(p1, [x + "/1" for x in names], r1, q1)
    _write_fastq(p2, [x + "/2" for x in names], r2, q2)
    want = fo.map_reads(c["ref"], c["idx"], fo.ReadBatch(r1 + r2), e=3, threads=THREADS)
    header = "".join("@SQ\tSN:s%d\tLN:%d\n" % (i, len(s)) for i, s in enumerate(c["seqs"]))
    out = tmp_path / "out.sam"
    r = _fem_map(c, p1, out, "--batch", "120", read2=p2)
    assert r.returncode == 0, r.stderr
    assert out.read_text(encoding="latin-1") == header + pm.sam_lines(want, n, ["s0", "s1"], r1 + r2, names + names, q1 + q2, 0, 2000)
    _, n_proper = pm.expected(want, n, 0, 2000)
    assert _counters(r.stderr) == _want_counters(want.stats) + ["The number of proper pairs: %d" % n_proper]
    assert n_proper > n // 4


PEEK_BYTES = 1 << 18  # FEM map sizes the device's reservation from the records in the input's first 256 KiB


@pytest.mark.parametrize("where", [0, 1500])
def test_fem_map_names_the_read_length_limit(cli_ref, tmp_path, where):
    # a read of 1025 bases first in the file, inside the records that size the device's reservation, or in a later batch
    # beyond them: the reservation made for 150-base reads, batches in flight in every slot, then the long read
    c = cli_ref
    rng = np.random.default_rng(4200 + where)
    reads = util.make_reads(rng, c["seqs"], 2000, 150, 3)
    reads[where] = util.make_reads(rng, c["seqs"], 1, MAX_LEN + 1, 3)[0]
    names = ["r%d" % i for i in range(len(reads))]
    fq = tmp_path / "reads.fq"
    _write_fastq(fq, names, reads, ["I" * len(r) for r in reads])
    before = fq.read_bytes().find(b"@%s c\n" % names[where].encode())
    if where:
        assert before > PEEK_BYTES + 4096, "fixture must put the long read beyond the records that size the reservation"
    else:
        assert before == 0
    r = _fem_map(c, fq, tmp_path / "out.sam", "--batch", "100")
    assert r.returncode == 1, r.stderr
    assert "read longer than the device path supports (1024)" in r.stderr, r.stderr
    assert "batch shape out of range" not in r.stderr
