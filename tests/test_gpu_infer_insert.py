"""The insert size estimate on the device (fem_dev_estimate_insert: insert_sample_kernel + insert_bounds_kernel, fem_tail.hip) and
FEM map --infer-insert against the plain-Python model of tests/insert_model.py on the oracle's single-end records of the same
reads.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import insert_model as im
from tests import util
from tests.cases import make_pairs, write_fastq
from tests.harness import build_index, open_reference, run_fem

pytestmark = pytest.mark.gpu

E = 3


class Case:
    def __init__(self, seed, repeats):
        self.rng, self.dev, self.ref, self.idx, self.seqs, self.names = open_reference(seed, repeats, 50_000, 7)

    def model(self, reads, e=E):
        """(the oracle's records, the model's estimate) of a batch of pairs (mate 1's reads, then mate 2's)."""
        res = fo.map_reads(self.ref, self.idx, fo.ReadBatch(reads), e=e, threads=4)
        return res, im.estimate(res, len(reads) // 2)

    def stage(self, reads, e=E, slot=0, text=False):
        batch = fo.ReadBatch(reads)
        self.dev.stage_reads(batch.bases, batch.off, slot=slot)
        if text:
            self.dev.stage_text(np.frombuffer(b"".join(b"I" * len(r) for r in reads), np.uint8), ["r%d" % (i % (len(reads) // 2)) for i in range(len(reads))],
                                slot=slot)
        self.dev.map_staged(e=e, slot=slot)

    def estimate(self, reads, e=E, slot=0):
        self.stage(reads, e, slot)
        return self.dev.estimate_insert(slot=slot)


@pytest.fixture(scope="module")
def plain():
    c = Case(601, False)
    c.dev.set_pairs(0, 500, slot=0)
    c.dev.set_pairs(0, 500, slot=1)
    yield c
    c.dev.close()


@pytest.fixture(scope="module")
def repeats():
    c = Case(602, True)
    c.dev.set_pairs(0, 500, slot=0)
    yield c
    c.dev.close()


def cut_pairs(seq, where, L=100):
    """Pairs cut out of seq without edits: (start, insert) -> mate 1 the fragment's first L bases, mate 2 the reverse complement of
    its last L, so that the insert is exactly what is asked for.  Every other pair has its mates swapped."""
    r1, r2 = [], []
    for k, (st, ins) in enumerate(where):
        a, b = seq[st:st + L], util.revcomp(seq[st + ins - L:st + ins])
        if k & 1:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    return r1, r2


def frag_pairs(rng, seq, frags, L, e):
    """Pairs from fragments of the given lengths, 0..e edits per mate (as make_pairs makes its concordant ones)."""
    def mut(s):
        s = util.mutate(rng, s, int(rng.integers(0, e + 1)))[:L]
        return s + util.rand_seq(rng, L - len(s)) if len(s) < L else s

    r1, r2 = [], []
    for frag in frags:
        frag = int(frag)
        st = int(rng.integers(0, len(seq) - frag - e - 1))
        f = seq[st:st + frag + e]
        a, b = mut(f[:L + e]), mut(util.revcomp(f[frag - L:frag + e][:L + e]))
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    return r1, r2


def random_mate_pairs(rng, seq, n, L=100):
    """Pairs of which one mate is random characters: never unique."""
    r1, r2 = cut_pairs(seq, [(1000 + 300 * k, 250) for k in range(n)], L)
    for k in range(n):
        if k % 3:
            r1[k] = util.rand_seq(rng, L)
        else:
            r2[k] = util.rand_seq(rng, L)
    return r1, r2


def _check(case, reads, e=E, slot=0):
    res, want = case.model(reads, e)
    got = case.estimate(reads, e, slot)
    assert got.as_tuple() == im.as_tuple(want), (got, want)
    return res, want


# ---- the estimate against the model ----

def test_generated_pairs_on_a_random_reference(plain):
    r1, r2 = make_pairs(plain.rng, plain.seqs, 1500, 100, E)
    _, want = _check(plain, r1 + r2)
    assert want["estimated"] and 800 < want["n_informative"] < want["n_unique"] < 1500  # (discordant kinds: unique, not informative)


def test_generated_pairs_on_a_repeat_rich_reference(repeats):
    r1, r2 = make_pairs(repeats.rng, repeats.seqs, 1500, 100, E)
    res, want = _check(repeats, r1 + r2)
    counts = np.diff(res.rec_off.astype(np.int64))
    assert int((counts > 1).sum()) > 300 and want["n_unique"] < 1200 and want["n_informative"] >= 64


def test_a_normal_library_with_a_few_far_pairs(plain):
    rng = np.random.default_rng(611)
    frags = np.clip(np.rint(rng.normal(300, 30, 1000)), 120, 600).astype(np.int64)
    r1, r2 = frag_pairs(rng, plain.seqs[0], list(frags) + [5000] * 6, 100, E)
    _, want = _check(plain, r1 + r2)
    assert want["n_informative"] > 500 and 270 <= want["q25"] < want["q50"] < want["q75"] <= 330
    assert 100 < want["min_insert"] < want["max_insert"] < 500  # the far pairs are counted and do not move the fence


def test_the_largest_insert(plain):
    where = [(2000 + 37 * k, im.INSERT_MAX + (k & 1)) for k in range(40)]  # 16383 and 16384 by turns
    r1, r2 = cut_pairs(plain.seqs[0], where)
    _, want = _check(plain, r1 + r2)
    assert (want["n_unique"], want["n_informative"], want["q25"], want["q75"]) == (40, 20, 16383, 16383)
    # among ordinary pairs: the bins' far end and their near end in one batch
    r1, r2 = cut_pairs(plain.seqs[0], where + [(30_000 + 211 * k, 100 + k) for k in range(100)])
    _, want = _check(plain, r1 + r2)
    assert (want["n_informative"], want["q25"], want["estimated"]) == (120, 129, 1)


def test_lower_case_reads(plain):
    rng = np.random.default_rng(613)
    r1, r2 = frag_pairs(rng, plain.seqs[0], rng.integers(200, 400, 600), 100, E)
    r1 = [r.lower() if i % 3 == 0 else r for i, r in enumerate(r1)]
    r2 = [r.lower() if i % 4 == 0 else r for i, r in enumerate(r2)]
    res, want = _check(plain, r1 + r2)
    counts = np.diff(res.rec_off.astype(np.int64))
    broken = [i for i in range(600) if counts[i] == 1 and counts[600 + i] == 1
              and (int(res.r_flag[int(res.rec_off[i])]) | int(res.r_flag[int(res.rec_off[600 + i])])) & 0x8000]
    assert len(broken) > 20 and want["n_unique"] <= 600 - len(broken) and want["n_informative"] >= 64


@pytest.mark.parametrize("n_pairs", [0, 1, 255, 256, 257])
def test_block_edges(plain, n_pairs):
    r1, r2 = cut_pairs(plain.seqs[0], [(500 + 301 * k, 150 + (53 * k) % 400) for k in range(n_pairs)])
    _, want = _check(plain, r1 + r2, slot=1)
    assert want["n_pairs"] == want["n_informative"] == n_pairs


def test_one_bin_takes_every_add(plain):
    r1, r2 = cut_pairs(plain.seqs[0], [(700 + 97 * k, 333) for k in range(1200)])
    _, want = _check(plain, r1 + r2)
    assert im.as_tuple(want) == (1200, 1200, 1200, 333, 333, 333, 333, 333, 1)


@pytest.mark.parametrize("n_informative", [63, 64])
def test_sixty_four_pairs_are_needed(plain, n_informative):
    rng = np.random.default_rng(617)
    a1, a2 = cut_pairs(plain.seqs[0], [(900 + 401 * k, 200 + 3 * k) for k in range(n_informative)])
    b1, b2 = random_mate_pairs(rng, plain.seqs[0], 30)
    _, want = _check(plain, a1 + b1 + a2 + b2)
    assert (want["n_pairs"], want["n_unique"], want["n_informative"], want["estimated"]) == (n_informative + 30, n_informative, n_informative,
                                                                                         int(n_informative == 64))
    assert (want["max_insert"] > 0) == (n_informative == 64)


# ---- what the call leaves alone ----

def test_later_fetches_and_the_timing_ids(plain):
    dev = plain.dev
    rng = np.random.default_rng(619)
    r1, r2 = make_pairs(rng, plain.seqs, 800, 100, E)
    reads = r1 + r2
    try:
        for slot in (0, 1):
            dev.set_rescue(4, slot=slot)
            dev.set_mapq(True, slot=slot)
            dev.set_unmapped(True, slot=slot)
            plain.stage(reads, slot=slot, text=True)
        dev.set_timing(True)
        dev.reset_timing()
        ids = range(17)
        count = lambda: [dev.kernel_time(k)[1] for k in ids]
        text0 = dev.fetch_sam(slot=0)[0]
        proper, rescued, unmapped = dev.pair_count(0), dev.rescue_count(0), dev.unmapped_count(0)
        assert rescued > 0 and unmapped > 0
        c0 = count()
        pairs0 = dev.fetch_pairs(slot=0)
        c1 = count()
        assert c1[16] == c0[16] == 0 and dev.kernel_time(16)[0] == 0.0  # neither a text nor the pairs count under the estimate's id
        got = dev.estimate_insert(slot=0)
        c2 = count()
        assert {k: c2[k] - c1[k] for k in ids if c2[k] != c1[k]} == {3: 1, 4: 1, 5: 1, 16: 1}
        assert dev.kernel_time(16)[0] > 0.0
        assert got.as_tuple() == im.as_tuple(plain.model(reads)[1])
        # none of the slot's counts, and the same text and pairs as before and as a slot that never made the call
        assert (dev.pair_count(0), dev.rescue_count(0), dev.unmapped_count(0)) == (pairs0.n_proper, rescued, unmapped)
        assert pairs0.n_proper == proper
        assert dev.fetch_sam(slot=0)[0] == text0 == dev.fetch_sam(slot=1)[0]
        again, other = dev.fetch_pairs(slot=0), dev.fetch_pairs(slot=1)
        for k in ("rec_begin", "flag", "tid", "pos0", "nm", "cigar_off", "cigar", "md_off", "md", "mate_tid", "mate_pos0", "tlen"):
            assert np.array_equal(getattr(again, k), getattr(pairs0, k)) and np.array_equal(getattr(other, k), getattr(pairs0, k)), k
        assert again.n_proper == other.n_proper == proper
        bam0 = dev.fetch_bam(slot=0, level=0)[0]
        dev.estimate_insert(slot=0)
        assert dev.fetch_bam(slot=0, level=0)[0] == bam0 == dev.fetch_bam(slot=1, level=0)[0]
    finally:
        dev.set_timing(False)
        for slot in (0, 1):
            dev.set_rescue(None, slot=slot)
            dev.set_mapq(False, slot=slot)
            dev.set_unmapped(False, slot=slot)


def test_refusals(plain):
    from fem_amd import FemError
    dev = plain.dev
    r1, r2 = cut_pairs(plain.seqs[0], [(500 + 301 * k, 300) for k in range(20)])
    dev.set_pairs(None, slot=2)
    plain.stage(r1 + r2, slot=2)
    with pytest.raises(FemError, match="pair mode"):
        dev.estimate_insert(slot=2)  # a single-end slot
    assert dev._L.fem_dev_estimate_insert(dev._h, 2, None) == -1  # FEM_ERR_INVALID: no result to fill
    dev.set_pairs(0, 500, slot=2)
    assert dev.estimate_insert(slot=2).n_informative == 20  # (the same batch: the slot's range is read at the call)
    plain.stage(r1 + r2[:-1], slot=2)
    with pytest.raises(FemError, match="even number"):
        dev.estimate_insert(slot=2)  # an odd number of reads
    dev.set_pairs(None, slot=2)


def test_the_slots_own_range_plays_no_part(plain):
    r1, r2 = cut_pairs(plain.seqs[0], [(500 + 301 * k, 600 + k) for k in range(100)])
    plain.dev.set_pairs(0, 100, slot=3)
    _, want = _check(plain, r1 + r2, slot=3)
    assert want["n_informative"] == 100 and want["q50"] == 649


# ---- FEM map --infer-insert ----

def _fastq(tmp, tag, r1, r2):
    base = ["%s%d" % (tag, i) for i in range(len(r1))]
    q1 = ["".join(chr(33 + (7 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r1)]
    q2 = ["".join(chr(34 + (5 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r2)]
    p1, p2 = tmp / (tag + "_1.fq"), tmp / (tag + "_2.fq")
    write_fastq(p1, r1, [b + "/1" for b in base], q1, False)
    write_fastq(p2, r2, [b + "/2" for b in base], q2, False)
    return p1, p2


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("infer")
    rng = np.random.default_rng(631)
    seqs = [util.rand_seq(rng, 150_000), util.rand_seq(rng, 60_000)]
    fa = tmp / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = tmp / "ref.idx"
    build_index(fa, idx_path)
    ref = fo.Reference(seqs)
    return dict(tmp=tmp, rng=rng, seqs=seqs, fa=fa, idx=idx_path, ref=ref, oidx=fo.OracleIndex(ref))


def _model(cli, r1, r2):
    res = fo.map_reads(cli["ref"], cli["oidx"], fo.ReadBatch(r1 + r2), e=E, threads=4)
    return im.estimate(res, len(r1))


def _map(cli, p1, p2, out, *extra, env=None):
    r = run_fem("map", "-e", E, "-t", "4", "--ref", cli["fa"], "--index", cli["idx"], "--read1", p1, "--read2", p2, "-o", out, *extra,
                env=env, text=True)
    assert r.returncode == 0, r.stderr
    return r.stderr.splitlines(), out.read_bytes()


def _inferred_line(m):
    return "Inferred insert size range: %d-%d (quartiles %d %d %d, %d informative of %d pairs)." % (
        m["min_insert"], m["max_insert"], m["q25"], m["q50"], m["q75"], m["n_informative"], m["n_pairs"])


def _insert_lines(stderr):
    return [l for l in stderr if "nsert size range" in l]


def test_cli_learns_the_range(cli):
    rng, tmp = np.random.default_rng(641), cli["tmp"]
    frags = np.clip(np.rint(rng.normal(300, 25, 2000)), 120, 600).astype(np.int64)
    frags[::50] = 470  # inside the default range, outside the learned one: the two runs differ
    r1, r2 = frag_pairs(rng, cli["seqs"][0], frags, 100, E)
    p1, p2 = _fastq(tmp, "a", r1, r2)
    m = _model(cli, r1, r2)
    assert m["estimated"] and 100 < m["min_insert"] and m["max_insert"] < 470
    lo, hi = str(m["min_insert"]), str(m["max_insert"])
    err, sam = _map(cli, p1, p2, tmp / "a.sam", "--infer-insert", "--batch", "700")
    assert _insert_lines(err) == [_inferred_line(m)]
    assert err.index(_inferred_line(m)) < min(i for i, l in enumerate(err) if l.startswith("Mapped read batch"))
    assert "The number of read: 4000" in err  # the sample is not counted
    err_x, sam_x = _map(cli, p1, p2, tmp / "ax.sam", "-I", lo, "-X", hi, "--batch", "700")
    assert sam == sam_x and not _insert_lines(err_x)
    assert [l for l in err if l.startswith("The number of")] == [l for l in err_x if l.startswith("The number of")]
    _, sam_default = _map(cli, p1, p2, tmp / "ad.sam", "--batch", "700")
    assert sam_default != sam
    # whatever the batches are
    assert _map(cli, p1, p2, tmp / "a1.sam", "--infer-insert", "--batch", "4000")[1] == sam
    # BAM
    _, bam = _map(cli, p1, p2, tmp / "a.bam", "--infer-insert", "--bam=0")
    _, bam_x = _map(cli, p1, p2, tmp / "ax.bam", "-I", lo, "-X", hi, "--bam=0")
    assert bam == bam_x and bam[:2] == b"\x1f\x8b"


def test_cli_learns_from_the_first_pairs_only(cli):
    rng, tmp = np.random.default_rng(643), cli["tmp"]
    frags = np.concatenate([rng.integers(190, 211, 128), rng.integers(390, 411, 600)])
    r1, r2 = frag_pairs(rng, cli["seqs"][0], frags, 100, E)
    p1, p2 = _fastq(tmp, "b", r1, r2)
    head, rest, whole = _model(cli, r1[:128], r2[:128]), _model(cli, r1[128:], r2[128:]), _model(cli, r1, r2)
    ranges = {(m["min_insert"], m["max_insert"]) for m in (head, rest, whole)}
    assert head["estimated"] and rest["estimated"] and len(ranges) == 3 and head["max_insert"] < 390
    err, sam = _map(cli, p1, p2, tmp / "b.sam", "--infer-insert=128", "--batch", "500")
    assert _insert_lines(err) == [_inferred_line(head)]
    assert "The number of read: %d" % (2 * len(r1)) in err
    assert sam == _map(cli, p1, p2, tmp / "bx.sam", "-I", str(head["min_insert"]), "-X", str(head["max_insert"]), "--batch", "500")[1]
    err, sam_all = _map(cli, p1, p2, tmp / "ball.sam", "--infer-insert", "--batch", "500")
    assert _insert_lines(err) == [_inferred_line(whole)] and sam_all != sam


def test_cli_falls_back_to_the_given_range(cli):
    rng, tmp = np.random.default_rng(647), cli["tmp"]
    a1, a2 = cut_pairs(cli["seqs"][0], [(900 + 401 * k, 200 + 9 * k) for k in range(40)])
    b1, b2 = random_mate_pairs(rng, cli["seqs"][0], 30)
    r1, r2 = a1 + b1, a2 + b2
    p1, p2 = _fastq(tmp, "c", r1, r2)
    m = _model(cli, r1, r2)
    assert (m["n_informative"], m["n_pairs"], m["estimated"]) == (40, 70, 0)
    err, sam = _map(cli, p1, p2, tmp / "c.sam", "--infer-insert")
    assert _insert_lines(err) == ["Insert size range not inferred (40 informative of 70 pairs, 64 needed): using 0-500."]
    assert sam == _map(cli, p1, p2, tmp / "cx.sam")[1]
    err, sam = _map(cli, p1, p2, tmp / "c2.sam", "--infer-insert", "-I", "250", "-X", "400")
    assert _insert_lines(err) == ["Insert size range not inferred (40 informative of 70 pairs, 64 needed): using 250-400."]
    assert sam == _map(cli, p1, p2, tmp / "c2x.sam", "-I", "250", "-X", "400")[1]


def test_cli_two_workers_and_every_paired_option(cli):
    rng, tmp = np.random.default_rng(653), cli["tmp"]
    r1, r2 = make_pairs(rng, cli["seqs"], 1500, 100, E)
    p1, p2 = _fastq(tmp, "d", r1, r2)
    m = _model(cli, r1, r2)
    assert m["estimated"]
    opts = ["--batch", "300", "--gpus", "2", "--rescue", "8", "--rescue-discordant", "--mapq", "--unmapped", "--nh"]
    share = {"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"}  # (two workers with a handle each on the one GPU)
    err, sam = _map(cli, p1, p2, tmp / "d.sam", "--infer-insert", *opts, env=share)
    err_x, sam_x = _map(cli, p1, p2, tmp / "dx.sam", "-I", str(m["min_insert"]), "-X", str(m["max_insert"]), *opts, env=share)
    assert _insert_lines(err) == [_inferred_line(m)]
    # (two workers' batches are written as they retire: the same bytes line for line, the batches in either run's own order)
    assert len(sam) == len(sam_x) and sorted(sam.splitlines()) == sorted(sam_x.splitlines())
    assert [l for l in err if l.startswith("The number of")] == [l for l in err_x if l.startswith("The number of")]
    # one worker: byte for byte
    one = [o for o in opts if o not in ("--gpus", "2")]
    assert len(one) == len(opts) - 2
    sam_1 = _map(cli, p1, p2, tmp / "d1.sam", "--infer-insert", *one)[1]
    assert sam_1 == _map(cli, p1, p2, tmp / "d1x.sam", "-I", str(m["min_insert"]), "-X", str(m["max_insert"]), *one)[1]
    assert sorted(sam_1.splitlines()) == sorted(sam.splitlines())
