"""The model of the lines for unmapped reads (tests/unmapped_model.py) on hand-built records: every row of the rule of
include/fem_hip.h (fem_dev_set_unmapped) at least once, and — on the oracle, without a GPU — that the case generators of
tests/cases.py (run by tests/test_gpu_unmapped.py) give what their cases need."""
from tests import bam_model as bm
from tests import cases
from tests import pair_model as pm
from tests import unmapped_model as um

SEQS = ["chrA", "chrB"]


def _lines(text):
    return [l.split("\t") for l in text.decode("latin-1").splitlines()]


def test_single_end_rows():
    # read 0: two records; read 1: unmapped; read 2: unmapped, of length 0; read 3: unmapped, odd letters; read 4: one record
    res = pm.Records([[(0, 0, 99, 0, [(5, "M")], "5"), (16 | 256, 1, 7, 1, [(5, "M")], "2A2")], [], [], [],
                      [(16, 1, 41, 2, [(2, "M"), (1, "I"), (2, "M")], "1C2")]])
    reads = [b"ACGTA", b"GGGTT", b"", b"acgNn.R0123u", b"TTTTT"]
    names = ["r0", "r1", "empty", "x" * 140, "r4"]
    quals = ["IIIII", "ABCDE", "", "!\"#$%&'()*+,", "55555"]
    text = um.single_end(res, SEQS, reads, names, quals)
    f = _lines(text)
    assert len(f) == 6
    assert f[0] == ["r0", "0", "chrA", "100", "255", "5M", "*", "0", "0", "ACGTA", "IIIII", "NM:i:0", "MD:Z:5"]
    assert f[1] == ["r0", "272", "chrB", "8", "255", "5M", "*", "0", "0", "*", "*", "NM:i:1", "MD:Z:2A2"]
    assert f[2] == ["r1", "4", "*", "0", "0", "*", "*", "0", "0", "GGGTT", "ABCDE"]
    assert f[3] == ["empty", "4", "*", "0", "0", "*", "*", "0", "0", "*", "*"]
    assert f[4] == ["x" * 140, "4", "*", "0", "0", "*", "*", "0", "0", "ACGNNNRACGTN", "!\"#$%&'()*+,"]
    assert f[5][:9] == ["r4", "16", "chrB", "42", "255", "2M1I2M", "*", "0", "0"]
    assert text.endswith(b"\t55555\tNM:i:2\tMD:Z:1C2\n") and b"\t\n" not in text
    # MAPQ: the mapped reads' lines get the rule's, an unmapped read's line 0 all the same
    q = [x[4] for x in _lines(um.single_end(res, SEQS, reads, names, quals, e=3))]
    assert q == ["20", "0", "0", "0", "0", "40"]
    # without the qualities QUAL is *; minus the FLAG & 4 lines the text is the default one
    assert _lines(um.single_end(res, SEQS, reads, names, None))[2][9:] == ["GGGTT", "*"]
    rest, removed = um.without_unmapped(text)
    assert removed == 3 and [x[0] for x in _lines(rest)] == ["r0", "r0", "r4"]
    # BAM: the unplaced record
    rec = bm.encode(b"\t".join(x.encode("latin-1") for x in f[2]), [b"chrA", b"chrB"])
    assert rec[4:12] == b"\xff" * 8 and rec[14:16] == (4680).to_bytes(2, "little") and len(rec) == 36 + 3 + 3 + 5


def _pair_records():
    """Pairs 0..4 (reads i and 5 + i): both mapped and proper; only mate 1, a0 reverse, a secondary line on another sequence;
    only mate 2, a0 forward; neither; both mapped, not concordant."""
    m = lambda flag, tid, pos, nm=0: (flag, tid, pos, nm, [(5, "M")], "5")
    return pm.Records([[m(0, 0, 100)], [m(16, 0, 300), m(256, 1, 50, 1)], [], [], [m(0, 0, 700)],
                       [m(16, 0, 250)], [], [m(0, 1, 400)], [], [m(0, 1, 900)]])


def test_pair_rows():
    res = _pair_records()
    reads = [b"AAAAA", b"CCCCC", b"GGGGG", b"", b"TTTTT", b"AACCA", b"acgtn", b"GGTTG", b"NNNNN", b"TTAAT"]
    names = ["p%d" % i for i in range(5)] * 2
    quals = ["%d%d%d%d%d" % ((i,) * 5) if len(r) else "" for i, r in enumerate(reads)]
    assert um.pair_classes(res, 5) == [2, 1, 1, 1]
    text = um.paired(res, 5, SEQS, reads, names, quals)
    f = _lines(text)
    assert [x[0] for x in f] == ["p0", "p0", "p1", "p1", "p1", "p2", "p2", "p3", "p3", "p4", "p4"]
    # pair 0: proper, untouched by the switch
    assert f[0][:9] == ["p0", str(0x1 | 0x2 | 0x20 | 0x40), "chrA", "101", "255", "5M", "=", "251", "155"]
    assert f[1][:9] == ["p0", str(0x1 | 0x2 | 0x10 | 0x80), "chrA", "251", "255", "5M", "=", "101", "-155"]
    # pair 1: A = mate 1 (a0 reverse on chrA at 300, a secondary line on chrB), B = mate 2 placed there
    assert f[2][:9] == ["p1", str(0x1 | 0x8 | 0x10 | 0x40), "chrA", "301", "255", "5M", "=", "301", "0"]
    assert f[3][:9] == ["p1", str(0x1 | 0x8 | 0x40 | 0x100), "chrB", "51", "255", "5M", "chrA", "301", "0"]
    assert f[4] == ["p1", str(0x1 | 0x4 | 0x20 | 0x80), "chrA", "301", "0", "*", "=", "301", "0", "ACGTN", "66666"]
    # pair 2: B = mate 1 placed at mate 2's forward record on chrB
    assert f[5] == ["p2", str(0x1 | 0x4 | 0x40), "chrB", "401", "0", "*", "=", "401", "0", "GGGGG", "22222"]
    assert f[6][:9] == ["p2", str(0x1 | 0x8 | 0x80), "chrB", "401", "255", "5M", "=", "401", "0"]
    # pair 3: neither maps; mate 1 has length 0
    assert f[7] == ["p3", "77", "*", "0", "0", "*", "*", "0", "0", "*", "*"]
    assert f[8] == ["p3", "141", "*", "0", "0", "*", "*", "0", "0", "NNNNN", "88888"]
    # pair 4: both map, not concordant: as without the switch
    assert f[9][:9] == ["p4", str(0x1 | 0x40), "chrA", "701", "255", "5M", "chrB", "901", "0"]
    # the default text is what is left without the FLAG & 4 lines, with * 0 back on the 0x8 lines
    rest, removed = um.without_unmapped(text, True)
    assert removed == 4 and rest.decode("latin-1") == pm.sam_lines(res, 5, SEQS, reads, names, quals)
    # MAPQ: A's lines as without the switch (q_se on the primary line), B's and the unplaced lines 0
    q = [x[4] for x in _lines(um.paired(res, 5, SEQS, reads, names, quals, e=3))]
    assert q[2:9] == ["20", "0", "0", "0", "60", "0", "0"]
    # BAM: the placed record has its mate's refID, pos and the bin of one base there
    rec = bm.encode(b"\t".join(x.encode("latin-1") for x in f[4]), [b"chrA", b"chrB"])
    assert rec[4:12] == (0).to_bytes(4, "little") + (300).to_bytes(4, "little")
    assert int.from_bytes(rec[14:16], "little") == bm.reg2bin(300, 301) and rec[24:32] == rec[4:12]
    assert bm.decode(rec, [b"chrA", b"chrB"])[0].decode("latin-1").split("\t") == f[4]


def test_a_rescued_mate_is_mapped():
    m = lambda flag, tid, pos, nm=0: (flag, tid, pos, nm, [(5, "M")], "5")
    se = pm.Records([[m(0, 0, 100)], []])
    reads, names, quals = [b"AAAAA", b"CCCCC"], ["p", "p"], ["IIIII", "JJJJJ"]
    off = _lines(um.paired(se, 1, SEQS, reads, names, quals, e=3))
    assert [x[1] for x in off] == [str(0x1 | 0x8 | 0x40), str(0x1 | 0x4 | 0x80)] and off[1][2:4] == ["chrA", "101"]
    assert off[0][6:8] == ["=", "101"] and [x[4] for x in off] == ["60", "0"]
    # the same pair with its mate 2 rescued at 240: a proper pair, nothing unmapped, no line of the switch
    withr = pm.Records([[m(0, 0, 100)], [m(16, 0, 240, 5)]])
    on = um.paired(se, 1, SEQS, reads, names, quals, e=3, res=withr, rescued={1})
    f = _lines(on)
    assert [int(x[1]) & 0xE for x in f] == [2, 2] and f[1][2:4] == ["chrA", "241"] and f[0][6:9] == ["=", "241", "145"]
    assert um.without_unmapped(on, True) == (on, 0)


# ---- the generators of the GPU cases meet their bounds (oracle and rescue model, no GPU) ----

def test_generated_single_end_cases():
    for case in cases.UNMAPPED_SINGLE_CASES:
        c = cases.unmapped_single_case(*case)
        cases.check_unmapped_single_case(c)


def test_generated_pair_cases():
    for case in cases.UNMAPPED_PAIR_CASES:
        c = cases.unmapped_pair_case(*case)
        cases.check_unmapped_pair_case(c)
