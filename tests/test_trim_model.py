"""The rule of read trimming in plain Python (tests/trim_model.py) on hand-written cases: the clip points, and what apply()
makes of a text.  The device and FEM map are held against this model in tests/test_gpu_trim.py.  No GPU."""
import numpy as np
import pytest

from tests import trim_model as m

GOOD, BAD = b"I", b"#"  # q = 40 and q = 2


def test_all_good_and_all_bad_qualities():
    assert m.clips(GOOD * 100, 0, 0, 20) == (0, 0)        # the first step is negative: stop, nothing cut
    assert m.clips(BAD * 100, 0, 0, 20) == (0, 65)        # every step raises the sum: down to the floor
    assert m.clips(BAD * 100, 0, 0, 0) == (0, 0)          # off
    assert m.clips(BAD * 1024, 0, 0, 1) == (0, 0)         # q = 2 against Q = 1: the sum falls at once
    assert m.clips(GOOD * 1024, 0, 0, 93) == (0, 1024 - 35)


def test_the_floor_of_35_bases():
    assert m.MIN_KEEP == 35
    assert m.clips(BAD * 35, 0, 0, 20) == (0, 0)          # L' = 35: no quality trim
    assert m.clips(BAD * 36, 0, 0, 20) == (0, 1)          # L' = 36: position 35 alone is looked at
    assert m.clips(BAD * 34, 0, 0, 20) == (0, 0)
    assert m.clips(BAD * 40, 3, 2, 20) == (3, 2)          # the floor counts what the fixed trims leave: L' = 35
    assert m.clips(BAD * 41, 3, 2, 20) == (3, 3)


def test_one_good_base_inside_a_bad_tail_stops_the_sum():
    # from the 3' end: three bad bases (+18 each = 54), one good one (-20 = 34, not below 0), then bad ones again
    q = GOOD * 60 + BAD * 5 + GOOD + BAD * 3
    assert m.clips(q, 0, 0, 20) == (0, 9)                 # 54, 34, 52, 70, 88, 106, 124: the maximum at the tail's start
    # three good ones in a row take the sum below zero: the stop; what lies in front of it is never seen
    q = GOOD * 50 + BAD * 10 + GOOD * 3 + BAD * 3
    assert m.clips(q, 0, 0, 20) == (0, 3)                 # 54, 34, 14, -6: stop; best was 54 at the last three
    q = GOOD * 50 + BAD * 10 + GOOD * 2 + BAD * 3
    assert m.clips(q, 0, 0, 20) == (0, 15)                # 54, 34, 14, then up again past 54


def test_ties_take_the_least_cut():
    at = bytes([33 + 20])                                 # q == Q: the sum stays
    assert m.clips(GOOD * 40 + at * 20, 0, 0, 20) == (0, 0)             # never above 0: nothing cut
    assert m.clips(GOOD * 40 + at * 10 + BAD * 4, 0, 0, 20) == (0, 4)   # 72 reached at the tail's start and kept along the plateau
    assert m.clips(GOOD * 40 + BAD * 2 + at * 5 + BAD * 2, 0, 0, 20) == (0, 9)  # a strictly larger sum further in wins


def test_bytes_below_33():
    q = GOOD * 40 + bytes([0, 10, 32])                    # q = -33, -23, -1: Q - q = 53, 43, 21
    assert m.clips(q, 0, 0, 20) == (0, 3)
    assert m.clips(GOOD * 40 + bytes([32]), 0, 0, 1) == (0, 1)


def test_fixed_trims():
    assert m.clips(GOOD * 100, 5, 7, 0) == (5, 7)
    assert m.clips(GOOD * 10, 8, 7, 0) == (8, 2)          # trim3 takes what trim5 leaves
    assert m.clips(GOOD * 10, 10, 7, 0) == (10, 0)
    assert m.clips(GOOD * 10, 1024, 1024, 20) == (10, 0)  # trim5 + trim3 >= L: nothing is kept
    assert m.clips(b"", 3, 4, 20) == (0, 0)               # L = 0
    assert m.clips(GOOD * 50 + BAD * 30, 2, 10, 20) == (2, 30)  # the quality trim goes on where trim3 stopped


def test_the_parallel_form_is_the_same_rule():
    rng = np.random.default_rng(1)
    for _ in range(300):
        L = int(rng.integers(0, 200))
        q = bytes(rng.choice([33 + 2, 33 + 20, 33 + 40, 33 + 19, 33 + 21, 10], size=L).astype(np.uint8))
        for t5, t3, Q in ((0, 0, 20), (3, 4, 20), (0, 0, 1), (60, 60, 2), (0, 0, 93)):
            assert m.clips(q, t5, t3, Q) == m.clips_parallel(q, t5, t3, Q)
    reads, quals = m.clip_case(2)
    assert all(m.clips(q.encode("latin-1"), 3, 4, 20) == m.clips_parallel(q.encode("latin-1"), 3, 4, 20) for q in quals)


def test_kept_and_counts():
    reads, quals = [b"ACGTACGTAC", b"", b"ACG"], ["IIIIIIIIII", "", "III"]
    kr, kq, cl = m.kept(reads, quals, 2, 3, 0)
    assert kr == [b"GTACG", b"", b""] and kq == ["IIIII", "", ""] and cl == [(2, 3), (0, 0), (2, 1)]
    assert m.counts(cl) == (2, 8)


def _line(name, flag, cigar, seq, qual, *tags):
    return b"\t".join([name, b"%d" % flag, b"chr", b"100", b"255", cigar, b"*", b"0", b"0", seq, qual] + list(tags)) + b"\n"


def test_apply_clips_forward_and_reverse_lines():
    reads, quals, cl = [b"AACCCGGGTT", b"TTACGTACAA"], ["0123456789", "abcdefghij"], [(2, 3), (1, 4)]
    base = _line(b"a", 0, b"5M", b"CCCGG", b"23456", b"NM:i:0") + _line(b"b", 16, b"2M1I2M", b"TACGT", b"bcdef", b"NM:i:1")
    want = (_line(b"a", 0, b"2S5M3S", b"AACCCGGGTT", b"0123456789", b"NM:i:0") +
            _line(b"b", 16, b"4S2M1I2M1S", b"TTACGTACAA", b"abcdefghij", b"NM:i:1"))  # the reverse line swaps the sides
    assert m.apply(base, reads, quals, cl, ["a", "b"]) == want
    turned = m.apply(base, reads, quals, cl, ["a", "b"], sam_seq=True).splitlines()[1].split(b"\t")
    assert turned[5] == b"4S2M1I2M1S" and turned[9] == b"TTGTACGTAA" and turned[10] == b"jihgfedcba"  # the whole read turned
    assert m.clipped_reverse_lines(want) == [want.splitlines()[1]]


def test_apply_star_cigars_secondary_lines_and_emptied_reads():
    reads, quals, cl = [b"acgtnacgt.", b"ACGTAC"], ["0123456789", "abcdef"], [(0, 2), (3, 3)]
    base = (_line(b"a", 0, b"*", b"ACGTNACG", b"01234567", b"NM:i:0") +      # a record without a CIGAR: * stays *
            _line(b"a", 256, b"8M", b"*", b"*", b"NM:i:1") +                  # a secondary line: clipped, and * * stay
            _line(b"a", 272, b"8M", b"*", b"*", b"NM:i:1") +
            _line(b"b", 4, b"*", b"*", b"*"))                                  # the emptied read is unmapped: L = 0 printed * *
    got = [l.split(b"\t") for l in m.apply(base, reads, quals, cl, ["a", "b"]).splitlines()]
    assert got[0][5] == b"*" and got[0][9] == b"ACGTNACGTN" and got[0][10] == b"0123456789"  # the letter table
    assert got[1][5] == b"8M2S" and got[1][9:11] == [b"*", b"*"]
    assert got[2][5] == b"2S8M" and got[2][9:11] == [b"*", b"*"]
    assert got[3][5] == b"*" and got[3][9] == b"ACGTAC" and got[3][10] == b"abcdef"          # ... and prints the whole read


def test_apply_mate_tags_and_xa_entries():
    # a pair: mate 1 forward, mate 2 reverse; MC is the other mate's clipped CIGAR, ms its whole qualities' score
    reads, quals, cl = [b"AACCCGG", b"TTTACGT"], ["5555555", "IIII###"], [(2, 0), (0, 3)]
    base = (_line(b"p", 99, b"5M", b"CCCGG", b"55555", b"NM:i:0", b"MC:Z:4M", b"MQ:i:255", b"ms:i:160",
                  b"XA:Z:chr,+7,5M,1;chr,-9,2M1D3M,2;") +
            _line(b"p", 147, b"4M", b"TTTA", b"IIII", b"NM:i:0", b"MC:Z:5M", b"MQ:i:255", b"ms:i:100"))
    got = [l.split(b"\t") for l in m.apply(base, reads, quals, cl, ["p"], paired=True).splitlines()]
    assert got[0][5] == b"2S5M" and got[0][12] == b"MC:Z:3S4M" and got[0][14] == b"ms:i:160"  # 4 * 40; the three # add nothing
    assert got[0][15] == b"XA:Z:chr,+7,2S5M,1;chr,-9,2M1D3M2S,2;"
    assert got[1][5] == b"3S4M" and got[1][12] == b"MC:Z:2S5M" and got[1][14] == b"ms:i:140"  # 7 * 20
    assert got[1][9] == b"TTTACGT" and got[1][10] == b"IIII###"


def test_the_cases_hold_what_the_gpu_tests_ask_of_them():
    c = m.tails_case()
    _, _, cl = m.kept(c["reads"], c["quals"], *c["trim"])
    assert [b for a, b in cl] == c["tails"] and len(c["reads"]) == 600 and set(len(r) for r in c["reads"]) == {120}
    assert sum(1 for t in c["tails"] if t >= 8) >= 400
    reads, quals = m.clip_case()
    assert set(len(r) for r in reads) == set(m.LENGTHS) and len(reads) == len(m.LENGTHS) * len(m.PROFILES) * 16
    assert any(min(q.encode("latin-1")) < 33 for q in quals if q)
    for trim in m.SETTINGS:
        assert m.counts(m.batch_clips(quals, *trim))[0] > 100
    g = m.ragged_case()
    kept = m.kept(g["reads"], g["quals"], *g["trim"])[0]
    assert sorted(len(r) for r in kept)[:3] == [0, 0, 28] and len(set(len(r) for r in kept)) > 30
    assert sum(1 for i, r in enumerate(g["reads"]) if i % 2) > 200  # every second read is a reverse-strand one


@pytest.mark.parametrize("kind", m.PROFILES)
def test_profiles_have_their_length(kind):
    rng = np.random.default_rng(2)
    for L in (0, 1, 36, 129):
        assert len(m.profile_quals(rng, kind, L, 3)) == L
