"""The model of the RG / NH / HI tags (tests/tags_model.py) on hand-written texts, and the hit-count case of tests/cases.py (run by
tests/test_gpu_tags.py), which has to hold slots of the sizes at which the kernels take another path.  No GPU."""
import struct

import numpy as np
import pytest

from tests import bam_model as bm
from tests import cases
from tests import tags_model as tm

REFS = [b"chr1", b"chr2"]


def _mapped(name, flag, pos=100, nm=0, seq=True, mate=b"*\t0\t0"):
    sq = b"ACGTACGTAC\tIIIIIIIIII" if seq else b"*\t*"
    return b"%s\t%d\tchr1\t%d\t255\t10M\t%s\t%s\tNM:i:%d\tMD:Z:10\n" % (name, flag, pos, mate, sq, nm)


def _unmapped(name, flag=4, at=b"*\t0", mate=b"*\t0\t0"):
    return b"%s\t%d\t%s\t0\t*\t%s\tACGTACGTAC\tIIIIIIIIII\n" % (name, flag, at, mate)


def _tail(line):  # the fields behind MD:Z (behind QUAL on an unmapped read's line)
    f = line.rstrip(b"\n").split(b"\t")
    return f[13:] if len(f) > 11 and f[11].startswith(b"NM:i:") else f[11:]


@pytest.mark.parametrize("k", [1, 9, 10, 99, 100])
def test_a_slot_of_k_lines(k):
    text = b"".join(_mapped(b"r", 0 if t == 0 else 256, pos=100 + t, seq=t == 0) for t in range(k))
    got = tm.apply(text, b"grp", True).split(b"\n")[:-1]
    assert len(got) == k
    for t, l in enumerate(got):
        assert _tail(l) == [b"NH:i:%d" % k, b"HI:i:%d" % (t + 1), b"RG:Z:grp"]
    assert tm.apply(text, None, True).split(b"\n")[k - 1].endswith(b"\tMD:Z:10\tNH:i:%d\tHI:i:%d" % (k, k))
    assert tm.apply(text, b"grp", False).split(b"\n")[0].endswith(b"\tMD:Z:10\tRG:Z:grp")
    assert tm.apply(text) == text


def test_one_line_literally():
    assert tm.apply(_mapped(b"r", 16), b"x y", True) == \
        b"r\t16\tchr1\t100\t255\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\tMD:Z:10\tNH:i:1\tHI:i:1\tRG:Z:x y\n"


def test_an_unmapped_line_between_mapped_ones():
    text = _mapped(b"a", 0) + _mapped(b"a", 256, 200, seq=False) + _unmapped(b"b") + _mapped(b"c", 16)
    got = [_tail(l) for l in tm.apply(text, b"g", True).split(b"\n")[:-1]]
    assert got == [[b"NH:i:2", b"HI:i:1", b"RG:Z:g"], [b"NH:i:2", b"HI:i:2", b"RG:Z:g"], [b"RG:Z:g"], [b"NH:i:1", b"HI:i:1", b"RG:Z:g"]]
    assert [_tail(l) for l in tm.apply(text, None, True).split(b"\n")[:-1]][2] == []  # never NH / HI on an unmapped read's line
    assert tm.apply(text, None, True).split(b"\n")[2] + b"\n" == _unmapped(b"b")


def test_a_pair_with_one_unmapped_mate():
    # mate 1 mapped twice (0x1 | 0x8 | 0x40), mate 2 placed at mate 1's first line (0x1 | 0x4 | 0x80)
    text = (_mapped(b"p", 73, mate=b"=\t100\t0") + _mapped(b"p", 73 | 256, 300, seq=False, mate=b"=\t100\t0") +
            _unmapped(b"p", 133, at=b"chr1\t100", mate=b"=\t100\t0"))
    got = [_tail(l) for l in tm.apply(text, b"g", True).split(b"\n")[:-1]]
    assert got == [[b"NH:i:2", b"HI:i:1", b"RG:Z:g"], [b"NH:i:2", b"HI:i:2", b"RG:Z:g"], [b"RG:Z:g"]]


def test_a_rescued_mate():
    # mate 1: three lines, the chosen one first; mate 2: the rescued record, its only line
    text = (_mapped(b"p", 99, mate=b"=\t300\t210") + _mapped(b"p", 99 | 256, 5000, seq=False, mate=b"=\t300\t0") +
            _mapped(b"p", 99 | 256, 9000, nm=2, seq=False, mate=b"=\t300\t0") + _mapped(b"p", 147, 300, nm=5, mate=b"=\t100\t-210"))
    got = [_tail(l) for l in tm.apply(text, None, True).split(b"\n")[:-1]]
    assert got == [[b"NH:i:3", b"HI:i:1"], [b"NH:i:3", b"HI:i:2"], [b"NH:i:3", b"HI:i:3"], [b"NH:i:1", b"HI:i:1"]]


def test_strip_undoes_apply():
    text = _mapped(b"a", 0) + _mapped(b"a", 256, 200, seq=False) + _unmapped(b"b") + _mapped(b"c", 16)
    for rg, hits in ((b"g", True), (None, True), (b"g", False), (None, False)):
        plain, tags = tm.strip(tm.apply(text, rg, hits))
        assert plain == text
        assert tags == [(2 if hits else None, 1 if hits else None, rg), (2 if hits else None, 2 if hits else None, rg), (None, None, rg),
                        (1 if hits else None, 1 if hits else None, rg)]


def test_bam_aux_by_hand():
    assert tm.aux(300, 7, b"lane 1") == b"NHI\x2c\x01\0\0HII\x07\0\0\0RGZlane 1\0"
    assert tm.aux(read_group=b"g") == b"RGZg\0" and tm.aux(1, 1) == b"NHI\1\0\0\0HII\1\0\0\0" and tm.aux() == b""
    assert tm.aux_decode(b"NMC\2MDZ4A5\0" + tm.aux(300, 7, b"g")) == [(b"NM", b"C", 2), (b"MD", b"Z", b"4A5"), (b"NH", b"I", 300),
                                                                       (b"HI", b"I", 7), (b"RG", b"Z", b"g")]
    text = tm.apply(_mapped(b"a", 0, nm=1) + _unmapped(b"b"), b"grp", True)
    recs = bm.records(tm.bam_payload(text, REFS))
    assert len(recs) == 2
    for rec in recs:
        assert struct.unpack_from("<i", rec)[0] == len(rec) - 4  # block_size includes the tags
    assert tm.record_aux(recs[0]) == b"NMC\1MDZ10\0NHI\1\0\0\0HII\1\0\0\0RGZgrp\0"
    assert tm.record_aux(recs[1]) == b"RGZgrp\0"  # an unmapped read's record: RG alone
    assert bm.bam_payload_to_sam(b"".join(recs), REFS) == text  # (the reader of tests.bam_model knows types I and Z)
    plain = tm.strip(text)[0]
    assert tm.bam_payload(plain, REFS) == bm.sam_to_bam_payload(plain, REFS)  # without tags: the records of tests.bam_model


def test_header_text():
    sq = b"@SQ\tSN:chr1\tLN:10\n@SQ\tSN:chr2\tLN:20\n"
    assert tm.header(sq) == b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + sq
    pg = tm.pg_line(["./FEM", "map", "--rg", "@RG\tID:a b", "-o", "x\ny"], "0.2")
    assert pg == b"@PG\tID:FEM\tPN:FEM\tVN:0.2\tCL:./FEM map --rg @RG\\tID:a b -o x y"
    assert tm.rg_line("@RG\\tID:x\tSM:y") == b"@RG\tID:x\tSM:y"
    assert tm.header(sq, tm.rg_line("@RG\\tID:x"), pg) == tm.HD + sq + b"@RG\tID:x\n" + pg + b"\n"


def test_the_asserted_case_has_the_records_it_is_for():
    c = tm.asserted_case()
    res = c["res"]
    flag, ro = res.r_flag.astype(np.int64), res.rec_off.astype(np.int64)
    slots = [flag[ro[r]:ro[r + 1]] for r in range(len(c["reads"]))]
    assert sum(1 for s in slots if len(s) == 0) >= 3  # unmapped reads
    assert sum(1 for s in slots if len(s) and not (s & 0x8000).any()) >= 5  # mapped plainly
    assert sum(1 for s in slots if len(s) == 1 and s[0] & 0x8000) >= 3  # the only line is a 0x8000 one
    assert sum(1 for s in slots if len(s) >= 3 and not s[0] & 0x8000 and (s[1:] & 0x8000).any()) >= 3  # ... among secondary lines
    assert len(c["reads"]) % 2 == 0  # (also taken as read pairs)


def test_the_hit_count_case_has_the_slots_it_is_for():
    c = cases.hits_case()
    counts = np.diff(c["res"].rec_off.astype(np.int64))
    assert set(counts.tolist()) == {1, 2, 130} and min(np.count_nonzero(counts == k) for k in (1, 2, 130)) >= 4
    order = [int(k) for k in counts]
    assert any(a != b for a, b in zip(order, order[1:]))  # mixed
