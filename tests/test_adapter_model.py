"""The rule of 3' adapter matching in plain Python (tests/adapter_model.py) on hand-written cases, its parallel form against the
serial one, and what the oracle makes of the read-through case with the adapter cut and without.  The device and FEM map are held
against this model in tests/test_gpu_adapter.py.  No GPU."""
import numpy as np

from oracle import fem_oracle as fo
from tests import adapter_model as m
from tests import trim_model as tm
from tests import util

A = b"AGATCGGAAGAGCACACGTC"  # 20 letters: E = 10 allows two mismatches in the whole of it
BODY = b"CCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCC"  # 40 letters that match no start of A within the thresholds below


def _mut(s, *at):
    s = bytearray(s)
    for p in at:
        s[p] = ord("T") if s[p] != ord("T") else ord("A")
    return bytes(s)


def test_the_adapter_whole_in_the_middle_of_the_read():
    assert m.cut(BODY + A + BODY, A) == 60
    assert m.cut(BODY + A, A) == 20
    assert m.cut(BODY, A) == 0


def test_the_adapter_at_the_very_end_around_the_least_overlap():
    for O in (3, 5, 8):
        assert m.cut(BODY + A[:O - 1], A, O, 0) == 0
        assert m.cut(BODY + A[:O], A, O, 0) == O
        assert m.cut(BODY + A[:O + 1], A, O, 0) == O + 1


def test_mismatches_at_the_threshold_and_one_above():
    assert m.cut(BODY + _mut(A, 3, 11), A) == 20          # 2 * 100 <= 20 * 10
    assert m.cut(BODY + _mut(A, 3, 11, 17), A) == 0       # 3 * 100 > 200; the starts behind it overlap too little of a match
    assert m.cut(BODY + _mut(A[:10], 4), A) == 10         # one in ten
    assert m.cut(BODY + _mut(A[:9], 4), A) == 0           # one in nine is over ten per cent
    assert m.cut(BODY + _mut(A, 3, 11, 17, 1, 7, 13), A, 5, 30) == 20  # 6 * 100 <= 20 * 30
    assert m.cut(BODY + _mut(A[:19], 3, 11, 17, 1, 7, 13), A, 19, 30) == 0  # 600 > 19 * 30


def test_no_errors_allowed():
    assert m.cut(BODY + A, A, 5, 0) == 20
    assert m.cut(BODY + _mut(A, 19), A, 20, 0) == 0
    assert m.cut(BODY + _mut(A, 19), A, 5, 0) == 0        # every shorter overlap starts inside A, where nothing matches exactly


def test_other_bytes_in_the_read_mismatch_every_letter():
    for odd in b"N=.nRy*":
        r = bytearray(BODY + A)
        r[45] = odd
        assert m.cut(bytes(r), A, 5, 0) == 0 and m.cut(bytes(r), A, 5, 10) == 20
    assert m.cut(b"NNNNNNNNNN", b"ACGT", 1, 30) == 0


def test_lower_case_reads_and_adapters():
    assert m.cut((BODY + A).lower(), A) == 20
    assert m.cut(BODY + A, A.lower()) == 20
    assert m.clips(BODY + A.lower(), "I" * 60, 0, 0, 0, A.lower()) == (0, 20, 20)


def test_a_read_that_is_all_adapter_keeps_nothing():
    assert m.cut(A, A) == 20 and m.cut(A[:7], A) == 7 and m.cut(A + BODY, A) == 60
    assert m.clips(A, "I" * 20, 0, 0, 20, A) == (0, 20, 20)


def test_empty_and_short_remainders():
    assert m.cut(b"", A) == 0                               # L' = 0
    assert m.cut(A[:4], A) == 0                             # L' < O
    assert m.clips(b"", "", 3, 4, 20, A) == (0, 0, 0)       # L = 0
    assert m.clips(A[:6], "IIIIII", 4, 2, 0, A) == (4, 2, 0)  # the fixed trims use the read up


def test_of_two_matches_the_left_one_wins():
    assert m.cut(BODY + A + BODY + A, A) == 80
    assert m.cut(BODY + A[:12] + BODY + A, A) == 20         # a partial copy in the middle is no match: its o is 20
    assert m.cut(BODY + _mut(A, 2, 9) + A, A) == 40         # the left one with two mismatches still is


def test_fixed_trims_in_front_of_the_match():
    r = BODY + A
    assert m.clips(r, "I" * 60, 0, 13, 0, A) == (0, 20, 7)   # trim3 cut the adapter's end: the overlap of 7 is what remains
    assert m.clips(r, "I" * 60, 0, 16, 0, A) == (0, 16, 0)   # ... of 4: below O, nothing more is cut
    assert m.clips(r, "I" * 60, 5, 0, 0, A) == (5, 20, 20)
    assert m.clips(A + BODY, "I" * 60, 3, 0, 0, A) == (3, 0, 0)  # trim5 took the adapter's start: A[3:] is no start of A


def test_the_quality_step_runs_on_the_remainder():
    # 60 bases in front of the adapter, the last 10 of them bad: the quality rule goes on where the adapter's cut stopped
    r, q = b"C" * 60 + A, "I" * 50 + "#" * 10 + "I" * 20
    assert m.clips(r, q, 0, 0, 20, A) == (0, 30, 20)
    assert m.clips(r, q, 0, 0, 20, None) == (0, 0, 0)        # as given the good adapter bases stop the sum at once
    # the floor of 35 is measured after the adapter's cut: 36 bases remain, one may go; 35 remain, none
    assert m.clips(b"C" * 36 + A, "#" * 56, 0, 0, 20, A) == (0, 21, 20)
    assert m.clips(b"C" * 35 + A, "#" * 55, 0, 0, 20, A) == (0, 20, 20)
    assert m.clips(b"C" * 35 + A, "#" * 55, 0, 0, 20, None) == (0, 20, 0)  # (without the adapter the floor is that of the whole read)
    assert tm.MIN_KEEP == 35


def test_kept_counts_and_pairs():
    reads, quals = [BODY + A, BODY, BODY + A2_TAIL, BODY + A], ["I" * 60, "I" * 40, "I" * 50, "I" * 60]
    kr, kq, cl, a3 = m.kept(reads, quals, 2, 0, 0, A, A2=A2_TAIL, paired=True)
    assert a3 == [20, 0, 10, 0] and cl == [(2, 20), (2, 0), (2, 10), (2, 0)]  # the second half is matched against the other adapter
    assert kr == [BODY[2:], BODY[2:], BODY[2:], BODY[2:] + A] and kq[0] == "I" * 38
    assert m.counts(a3) == (2, 30) and tm.counts(cl) == (4, 38)
    assert m.batch_clips(reads, quals, 2, 0, 0, A)[1] == [20, 0, 0, 20]


A2_TAIL = b"GGTTGGTTGG"


def test_the_parallel_form_is_the_same_rule():
    rng = np.random.default_rng(1)
    full = util.rand_seq(rng, 64)
    n = 0
    for L in tm.LENGTHS:
        for k in range(3 if L > 200 else 8):
            ma = m.ADAPTERS[int(rng.integers(0, len(m.ADAPTERS)))]
            r = bytearray(util.rand_seq(rng, L))
            if L:
                p = int(rng.integers(0, L))
                part = bytearray(full[:min(ma, L - p)])
                for j in rng.choice(len(part), min(len(part), int(rng.integers(0, 4))), replace=False):
                    part[j] = ord("N")
                r[p:p + len(part)] = part
            for O, E in ((5, 10), (1, 0), (4, 30), (ma, 0)):
                want = m.cut(bytes(r), full[:ma], min(O, ma), E)
                assert m.cut_parallel(bytes(r), full[:ma], min(O, ma), E) == want == m.cut_np(bytes(r), full[:ma], min(O, ma), E)
                n += want > 0
    assert n > 100


def test_the_read_through_case_maps_with_the_adapter_cut_and_not_without():
    c = m.readthrough_case()
    assert len(c["reads"]) == 600 and set(len(r) for r in c["reads"]) == {120} and max(c["through"]) == 47
    kept, _, cl, a3 = m.kept(c["reads"], c["quals"], 0, 0, 0, c["adapter"])
    exact = sum(1 for a, t in zip(a3, c["through"]) if a == t)
    short = sum(1 for a, t in zip(a3, c["through"]) if a == 0 and 1 <= t <= 4)
    print("cut exactly the read-through: %d of 600; 1 to 4 adapter bases, nothing cut: %d; cut longer: %d"
          % (exact, short, sum(1 for a, t in zip(a3, c["through"]) if a > t)))
    assert exact + short >= 590 and all(a == t for a, t in zip(a3, c["through"]) if t >= 8)
    long_ = [i for i, t in enumerate(c["through"]) if t >= 8]
    whole = fo.map_reads(c["ref"], c["idx"], fo.ReadBatch(c["reads"]), e=c["e"], threads=8)
    cut = fo.map_reads(c["ref"], c["idx"], fo.ReadBatch(kept), e=c["e"], threads=8)
    on = sum(1 for i in long_ if cut.rec_off[i + 1] > cut.rec_off[i]) / len(long_)
    off = sum(1 for i in long_ if whole.rec_off[i + 1] > whole.rec_off[i]) / len(long_)
    print("reads with a read-through >= 8: %d; with a line: %.3f with the adapter cut, %.3f without" % (len(long_), on, off))
    assert len(long_) >= 400 and on >= 0.90 and off <= 0.10


def test_chance_cuts_on_random_reads_are_rare():
    rng = np.random.default_rng(9)
    cuts = [m.cut_np(util.rand_seq(rng, 100), m.A1) for _ in range(20000)]
    n = sum(1 for x in cuts if x)
    print("chance cuts: %d of 20000 reads, %d bases, at most %d from one read" % (n, sum(cuts), max(cuts)))
    assert n <= 0.005 * 20000


def test_the_cases_hold_what_the_gpu_tests_ask_of_them():
    full, reads, quals = m.match_case()
    assert 1500 <= len(reads) <= 2500 and set(tm.LENGTHS) <= set(len(r) for r in reads)
    for ma in m.ADAPTERS:
        a3 = m.batch_clips(reads, quals, 0, 0, 0, full[:ma], min(5, ma), 10)[1]
        starts = set((len(r) - a) % 64 for r, a in zip(reads, a3) if a)
        assert m.counts(a3)[0] > 100 and starts == set(range(64))  # matches at every lane, the windows' ends among them
        assert any(a == len(r) > 0 for r, a in zip(reads, a3))      # a read that is all adapter
    p = m.pairs_case()
    assert sum(1 for f in p["frag"] if f < 112) > 100 and sum(1 for f in p["frag"] if f >= 120) > 50
    a3 = m.batch_clips(p["reads"], p["quals"], 0, 0, 0, p["adapter"], A2=p["adapter2"], paired=True)[1]
    assert all(a == max(0, 120 - f) or 120 - f < 5 for a, f in zip(a3, p["frag"] + p["frag"]))
    only1 = m.batch_clips(p["reads"], p["quals"], 0, 0, 0, p["adapter"], paired=True)[1]
    assert only1[:300] == a3[:300] and sum(1 for a, b in zip(only1[300:], a3[300:]) if a != b) > 50  # mate 2 needs its own adapter
