"""tests/coverage_model.py against bins worked out by hand, and the library's symbols the feature adds.  No GPU."""
import numpy as np

from tests import coverage_model as m

NAMES, LENS = ["chrA", "chrB"], [30, 23]


def _line(flag, rname, pos1, cigar, mapq=255, tags=()):
    f = [b"r", b"%d" % flag, rname, b"%d" % pos1, b"%d" % mapq, cigar, b"*", b"0", b"0", b"ACGT", b"IIII", b"NM:i:0", b"MD:Z:4"]
    return b"\t".join(f + list(tags)) + b"\n"


def _bins(text, window, **kw):
    return m.bins(text, NAMES, LENS, window, **kw).tolist()


def test_span_inside_one_window():
    # bases 12 .. 16 of chrA at W = 10: all five in window [10, 20)
    assert _bins(_line(0, b"chrA", 13, b"5M"), 10) == [0, 5, 0, 0, 0, 0]


def test_span_across_a_boundary():
    # bases 8 .. 13: two in [0, 10), four in [10, 20)
    assert _bins(_line(16, b"chrA", 9, b"6M"), 10) == [2, 4, 0, 0, 0, 0]


def test_span_across_five_windows_at_w7():
    # bases 5 .. 29 of chrA (25M), W = 7: windows [0,7) 2, [7,14) 7, [14,21) 7, [21,28) 7, [28,30) 2; chrB has ceil(23 / 7) = 4
    assert _bins(_line(0, b"chrA", 6, b"25M"), 7) == [2, 7, 7, 7, 2, 0, 0, 0, 0]


def test_span_ends_on_the_last_base_of_a_short_last_window():
    # chrB has 23 bases: windows [0,10) [10,20) [20,23); bases 18 .. 22
    assert _bins(_line(0, b"chrB", 19, b"5M"), 10) == [0, 0, 0, 0, 2, 3]
    assert m.layout(LENS, 10) == [0, 3, 6] and m.layout(LENS, 7) == [0, 5, 9] and m.layout([1, 8, 9], 8) == [0, 1, 2, 4]


def test_second_sequence_offset_and_w1():
    got = _bins(_line(0, b"chrB", 1, b"3M"), 1)
    assert len(got) == 53 and got[30:33] == [1, 1, 1] and sum(got) == 3


def test_deletion_counts_and_insertion_does_not():
    # 10M2D20M from base 0 of chrA covers 32 reference bases, cut at the sequence's 30; 10M3I20M covers 30
    assert m.span(b"10M2D20M") == 32 and m.span(b"10M3I20M") == 30 and m.span(b"*") is None
    assert _bins(_line(0, b"chrB", 1, b"10M2D8M"), 10) == [0, 0, 0, 10, 10, 0]
    assert _bins(_line(0, b"chrB", 1, b"10M3I8M"), 10) == [0, 0, 0, 10, 8, 0]
    assert _bins(_line(0, b"chrA", 1, b"10M2D20M"), 10) == [10, 10, 10, 0, 0, 0]


def test_soft_clips_do_not_enter():
    # POS is that of the first aligned base: 3S5M2S at POS 13 covers bases 12 .. 16
    assert _bins(_line(0, b"chrA", 13, b"3S5M2S"), 10) == [0, 5, 0, 0, 0, 0]


def test_lines_that_do_not_count():
    text = _line(4, b"chrA", 13, b"*") + _line(256, b"chrA", 13, b"5M") + _line(0, b"chrA", 13, b"*") + _line(77, b"*", 0, b"*")
    assert _bins(text, 10) == [0] * 6
    assert _bins(text, 10, all_hits=True) == [0, 5, 0, 0, 0, 0]  # the secondary line alone


def test_mapq_threshold():
    text = _line(0, b"chrA", 1, b"4M", mapq=29) + _line(0, b"chrA", 11, b"4M", mapq=30) + _line(256, b"chrA", 21, b"4M", mapq=60)
    assert _bins(text, 10, min_mapq=30) == [0, 4, 0, 0, 0, 0]
    assert _bins(text, 10, min_mapq=30, all_hits=True) == [0, 4, 4, 0, 0, 0]
    assert _bins(text, 10, min_mapq=0) == [4, 4, 0, 0, 0, 0]


def test_xa_entries_count_with_all_hits_only():
    text = _line(0, b"chrA", 1, b"4M", tags=[b"XA:Z:chrB,-11,2S6M,1;chrA,+21,*,0;"])
    assert _bins(text, 10) == [4, 0, 0, 0, 0, 0]
    assert _bins(text, 10, all_hits=True) == [4, 0, 0, 0, 6, 0]  # chrB bases 10 .. 15; the * entry adds nothing


def test_bed_text():
    track = np.array([1, 80, 0, 9], np.uint64)  # W = 8 over 1, 8 and 9 bases
    assert m.bed(["a", "bb", "c"], [1, 8, 9], 8, track) == b"a\t0\t1\t1\t1.00\nbb\t0\t8\t80\t10.00\nc\t0\t8\t0\t0.00\nc\t8\t9\t9\t9.00\n"


def test_symbols():
    from fem_amd import device
    from tests import cases
    new = {"fem_dev_set_coverage", "fem_dev_coverage_layout", "fem_dev_fetch_coverage", "fem_dev_reset_coverage", "fem_dbg_stage_ms"}
    assert new <= set(device.ABI_SYMBOLS) & set(cases.declared_symbols())
