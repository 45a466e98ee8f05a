"""The rule of the mates' overlap in plain Python (tests/overlap_model.py) on hand-written cases, its three forms against one
another, its composition with the adapter and the quality trim against trimming by hand, and the conditions the cases of
tests/test_gpu_overlap.py rest on.  The device and FEM map are held against this model there.  No GPU."""
import numpy as np

from tests import adapter_model as am
from tests import overlap_model as m
from tests import trim_model as tm
from tests import util

RNG = np.random.default_rng(2)
FRAGMENT = util.rand_seq(RNG, 60)
J1, J2 = util.rand_seq(RNG, 40), util.rand_seq(RNG, 40)  # what follows the fragment in either mate


def _mut(s, *at):
    s = bytearray(s)
    for p in at:
        s[p] = ord("T") if s[p] != ord("T") else ord("A")
    return bytes(s)


def _pair(f, L1=100, L2=100):
    return (FRAGMENT[:f] + J1 + J2)[:L1], (util.revcomp(FRAGMENT[:f]) + J2 + J1)[:L2]


def test_a_fragment_shorter_than_both_mates_is_found():
    x, y = _pair(60)
    assert m.frag(x, y) == 60 and m.cuts(100, 100, 60) == (40, 40)
    assert m.frag(x, util.rand_seq(RNG, 100)) == 0 and m.cuts(100, 100, 0) == (0, 0)


def test_one_read_through_base_is_enough():
    x, y = _pair(59, 60, 60)
    assert m.frag(x, y) == 59 and m.cuts(60, 60, 59) == (1, 1)
    x, y = FRAGMENT, util.revcomp(FRAGMENT)  # the fragment is the read: no candidate below max(L) matches
    assert m.frag(x, y) == 0


def test_the_one_sided_read_through():
    x, y = _pair(60, 100, 40)  # mate 2 ends inside the fragment: only mate 1 is cut
    assert m.frag(x, y) == 60 and m.cuts(100, 40, 60) == (40, 0)
    x, y = _pair(60, 40, 100)
    assert m.frag(x, y) == 60 and m.cuts(40, 100, 60) == (0, 40)


def test_the_overlap_around_the_least_one():
    for O in (8, 12, 20):
        for o, want in ((O - 1, 0), (O, 50), (O + 1, 50)):
            x, y = _pair(50, 100, o)  # o = min(f, L1') - max(0, f - L2') = L2'
            assert m.frag(x, y, O, 0) == want
            assert m.frag(*_pair(o, 100, 100), O, 0) == (o if want else 0)  # ... and o = f


def test_mismatches_at_the_threshold_and_one_above():
    x, y = _pair(60)
    assert m.frag(_mut(x, 3, 11, 17, 31, 44, 59), y) == 60            # 6 * 100 <= 60 * 10
    assert m.frag(_mut(x, 3, 11, 17, 31, 44, 59, 20), y) == 0         # 7 * 100 > 600
    assert m.frag(_mut(x, 3), _mut(y, 3), 20, 10) == 60               # one in each mate, at places that are not aligned
    assert m.frag(_mut(x, *range(0, 36, 2)), y, 12, 30) == 60         # 18 * 100 <= 60 * 30
    assert m.frag(_mut(x, *range(0, 38, 2)), y, 12, 30) == 0
    assert m.frag(_mut(x, 7), y, 8, 0) == 0 and m.frag(x, y, 8, 0) == 60


def test_other_bytes_match_nothing_even_when_aligned():
    x, y = _pair(60)
    for odd in b"N=.nRy*":
        bx, by = bytearray(x), bytearray(y)
        bx[10] = by[60 - 1 - 10] = odd  # the same place of the fragment in both mates
        assert m.frag(bytes(bx), bytes(by), 20, 0) == 0 and m.frag(bytes(bx), bytes(by), 20, 10) == 60
        assert m.frag(bytes(bx), y, 20, 0) == 0 and m.frag(x, bytes(by), 20, 0) == 0
    assert m.frag(b"N" * 50, b"N" * 50, 8, 30) == 0


def test_lower_case_is_a_letter():
    x, y = _pair(60)
    assert m.frag(x.lower(), y) == m.frag(x, y.lower()) == m.frag(x.lower(), y.lower()) == 60


def test_in_a_tandem_repeat_the_largest_candidate_wins():
    fragment = b"ACGTT" * 12
    x, y = fragment + J1, util.revcomp(fragment) + J2
    matching = [f for f in range(1, 100) if m.frag(x[:f + 1], y[:f + 1], 20, 0) == f]  # every f that matches on its own
    assert m.frag(x, y, 20, 0) == 60 and len([f for f in matching if f < 60]) >= 5


def test_empty_and_short_mates():
    assert m.frag(b"", b"") == 0 and m.frag(b"", FRAGMENT) == 0 and m.frag(FRAGMENT, b"") == 0 and m.frag(b"A", b"T") == 0
    assert m.batch_clips([b"", b""], ["", ""], 3, 4, 20) == ([(0, 0), (0, 0)], [0, 0], [0, 0])
    x, y = _pair(10, 30, 30)
    assert m.frag(x, y, 8, 0) == 10 and m.cuts(30, 30, 10) == (20, 20)  # every mate keeps O bases at the least


def test_the_three_forms_are_the_same_rule():
    reads, quals = m.match_case()
    n = len(reads) // 2
    rng = np.random.default_rng(3)
    small = [i for i in range(n) if max(len(reads[i]), len(reads[n + i])) <= 200]
    large = [i for i in range(n) if max(len(reads[i]), len(reads[n + i])) >= 1023]
    cut = 0
    for i in list(rng.choice(small, 150, replace=False)) + list(rng.choice(large, 3, replace=False)):
        for O, E in m.SETTINGS[:3] if i in small else m.SETTINGS[:1]:
            want = m.frag(reads[i], reads[n + i], O, E)
            assert m.frag_parallel(reads[i], reads[n + i], O, E) == want == m.frag_np(reads[i], reads[n + i], O, E)
            cut += want > 0
    assert cut > 100
    for t5, t3, Q in m.TRIMS[1:2]:  # behind fixed trims, through batch_clips
        picked = sorted(int(i) for i in rng.choice(small, 60, replace=False))
        sub = [reads[i] for i in picked] + [reads[n + i] for i in picked]
        subq = [quals[i] for i in picked] + [quals[n + i] for i in picked]
        assert m.batch_clips(sub, subq, t5, t3, Q, frag=m.frag) == m.batch_clips(sub, subq, t5, t3, Q, frag=m.frag_parallel) == m.batch_clips(sub, subq, t5, t3, Q)


def test_the_composition_with_adapter_and_quality_trim_is_trimming_by_hand():
    A = am.A1
    x = FRAGMENT[:50] + A + J1          # 50 + 33 + 40 = 123: the fragment, mate 1's adapter, more
    y = util.revcomp(FRAGMENT[:50]) + J2  # 90: no adapter here, the overlap alone says where mate 2 ends
    quals = ["I" * 40 + "#" * 10 + "I" * 73, "I" * 90]
    # by hand: the overlap finds F = 50: v3 = (73, 40); the adapter is found at 50 in mate 1 only: a3 = (73, 0); the larger of the
    # two comes off; the quality rule runs on the 50 bases left, whose last 10 are bad
    cl, v3, a3 = m.batch_clips([x, y], quals, 0, 0, 20, A=A)
    assert (v3, a3) == ([73, 40], [73, 0]) and cl == [(0, 83), (0, 40)]
    assert m.batch_clips([x, y], quals, 0, 0, 0, A=A)[0] == [(0, 73), (0, 40)]
    assert m.batch_clips([x, y], quals, 0, 0, 0)[0] == [(0, 73), (0, 40)]
    # the adapter's cut is the larger: a copy of the adapter inside the fragment, at 30
    inner = FRAGMENT[:30] + A
    x2, y2 = inner + J1[:27], util.revcomp(inner) + J2[:27]
    cl, v3, a3 = m.batch_clips([x2, y2], ["I" * 90] * 2, 0, 0, 0, A=A, A2=b"TTTTGGGGTTTTGGGG")
    assert v3 == [27, 27] and a3 == [60, 0] and cl == [(0, 60), (0, 27)]
    # fixed trims in front: both mates lose 3 bases of the fragment's two ends, the fragment of the rule is the 44 between them
    cl, v3, a3 = m.batch_clips([x, y], quals, 3, 4, 0)
    assert v3 == [123 - 7 - 44, 90 - 7 - 44] and cl == [(3, 4 + 72), (3, 4 + 39)]
    kr, kq, cl, v3, a3 = m.kept([x, y], quals, 0, 0, 20, A=A)
    assert kr == [FRAGMENT[:40], util.revcomp(FRAGMENT[:50])] and kq == ["I" * 40, "I" * 50]
    assert m.counts(v3) == (1, 113) and tm.counts(cl) == (2, 123) and am.counts(a3) == (1, 73)


def test_the_pairs_case_is_cut_at_the_fragment_and_random_pairs_are_not():
    p = am.pairs_case()
    assert len(p["frag"]) == 300 and min(p["frag"]) >= 73 and max(p["frag"]) <= 160
    v3 = m.batch_clips(p["reads"], p["quals"], 0, 0, 0, 20, 10)[1]
    short = [i for i in range(300) if p["frag"][i] < 120]
    assert len(short) == 160
    assert all(v3[i] == v3[300 + i] == 120 - p["frag"][i] for i in short)
    assert all(v3[i] == v3[300 + i] == 0 for i in range(300) if p["frag"][i] >= 120)
    assert m.counts(v3) == (160, 2 * sum(120 - p["frag"][i] for i in short))
    # a read-through of 1 to 4 bases: the adapter at its default overlap of 5 sees nothing, the overlap does
    a3 = am.batch_clips(p["reads"], p["quals"], 0, 0, 0, am.A1, A2=am.A2, paired=True)[1]
    few = [i for i in range(300) if 116 <= p["frag"][i] <= 119]
    assert len(few) >= 5 and all(a3[i] == a3[300 + i] == 0 and v3[i] == 120 - p["frag"][i] for i in few)
    r = m.random_pairs()
    assert len(r) == 10000 and set(len(x) for x in r) == {100}
    for O in (20, 12, 8):
        assert m.counts(m.batch_clips(r, [""] * len(r), 0, 0, 0, O, 10)[1]) == (0, 0)


def test_the_match_case_holds_what_the_gpu_tests_ask_of_it():
    reads, quals = m.match_case()
    n = len(reads) // 2
    assert 1300 <= n <= 1700
    L1, L2 = [len(r) for r in reads[:n]], [len(r) for r in reads[n:]]
    assert set(zip(L1, L2)) >= set((a, b) for a in tm.LENGTHS for b in tm.LENGTHS)  # every length with every other
    v3 = m.batch_clips(reads, quals, 0, 0, 0, 20, 10)[1]
    F = [max(a, b) - (v3[i] if a >= b else v3[n + i]) if v3[i] + v3[n + i] else 0 for i, (a, b) in enumerate(zip(L1, L2))]
    lanes = set((max(a, b) - 1 - f) % 64 for a, b, f in zip(L1, L2, F) if f)
    assert lanes == set(range(64))                                                  # matches at every lane of a window
    assert {0, 1, -1, 63, 64, 65} <= set(b - f for b, f in zip(L2, F) if f)         # the shifts of z against x
    assert any(f == max(a, b) - 1 for a, b, f in zip(L1, L2, F) if f)               # the first candidate
    assert any(min(a, b) < f < max(a, b) and a > b for a, b, f in zip(L1, L2, F)) and any(min(a, b) < f < max(a, b) and a < b for a, b, f in zip(L1, L2, F))
    assert any(max(a, b) == 1024 and f for a, b, f in zip(L1, L2, F))
    for O, E in m.SETTINGS[:3]:
        got = m.counts(m.batch_clips(reads, quals, 0, 0, 0, O, E)[1])
        assert got[0] > 300, (O, E, got)
    assert m.counts(m.batch_clips(reads, quals, 0, 0, 0, *m.SETTINGS[3])[1]) == (0, 0)
    # the settings tell the cases apart: the thresholds of E and the odd bytes decide pairs
    by = [m.batch_clips(reads, quals, 0, 0, 0, O, E)[1] for O, E in m.SETTINGS[:3]]
    assert sum(1 for a, b in zip(by[0], by[1]) if a and not b) > 50 and sum(1 for a, b in zip(by[0], by[2]) if b and not a) > 50
