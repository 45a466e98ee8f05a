"""Paired-end mapping, the parts that need no GPU: FEM map's new options and their checks, the record-count reader that cuts
the second read file (fem_seqfile_plan_count), and the output rules of tests/pair_model.py on hand-built record lists."""
import gzip

import numpy as np
import pytest

from fem_amd import host
from tests import pair_model as pm
from tests import util
from tests.cases import bgzf
from tests.harness import run_fem



@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def run(*args):
    return run_fem(*args, text=True)


def test_usage_lists_the_pair_options():
    r = run("map", "-h")
    for opt in ("--read2", "-I", "-X"):
        assert opt in r.stderr


@pytest.mark.parametrize("ins", [("-I", "600", "-X", "500"), ("-I", "-1"), ("-X", str((1 << 30) + 1)),
                                 ("--minins", "10", "--maxins", "9")])
def test_bad_insert_size_range_is_refused(tmp_path, ins):
    args = ["map", "-e", "3", "--ref", str(tmp_path / "x.fa"), "--index", str(tmp_path / "x.idx"), "--read1",
            str(tmp_path / "r1.fq"), "--read2", str(tmp_path / "r2.fq"), "-o", str(tmp_path / "o.sam")] + list(ins)
    r = run(*args)
    assert r.returncode == 1 and "Wrong insert size range." in r.stderr
    r = run(*[a for a in args if a not in ("--read2", str(tmp_path / "r2.fq"))])  # checked without --read2 as well
    assert r.returncode == 1 and "Wrong insert size range." in r.stderr


def _fastq(tmp_path, n):
    rng = np.random.default_rng(5)
    recs = []
    for i in range(n):
        ln = 100 if i % 9 else int(rng.integers(1, 180))
        recs.append(b"@r%d/1 c\n" % i + util.rand_seq(rng, ln) + b"\n+\n" + bytes(rng.integers(33, 74, size=ln).astype(np.uint8)) + b"\n")
    recs.insert(7, b"@empty\n\n+\n\n")  # zero-length: skipped, not counted
    data = b"".join(recs)
    plain = tmp_path / "r.fq"
    plain.write_bytes(data)
    gz = tmp_path / "r.fq.gz"
    with gzip.open(str(gz), "wb", compresslevel=1) as f:
        f.write(data)
    bg = tmp_path / "r.fq.bgz.gz"
    bg.write_bytes(bgzf(data))
    return plain, gz, bg


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("per", [1, 777, 4000])
def test_plan_count_cuts_the_file_by_records(tmp_path, kind, per):
    n = 12_000
    path = _fastq(tmp_path, n)[kind]
    whole = host.read_sequences(str(path))
    assert whole.n == n
    counts = [per] * ((n + per - 1) // per) + [per, 5]
    parts = host.read_counted_batches(str(path), counts, threads=4)
    want, left = [], n
    for c in counts:
        want.append(min(c, left))
        left -= want[-1]
    assert [p.n for p in parts] == want and want[-2:] == [0, 0]
    got = [(p.name(i), p.seq(i), p.qual(i)) for p in parts for i in range(p.n)]
    assert got == [(whole.name(i), whole.seq(i), whole.qual(i)) for i in range(n)]


def test_plan_count_after_byte_plans_and_at_the_end(tmp_path):
    plain, gz, bg = _fastq(tmp_path, 3000)
    for path in (plain, gz, bg):
        whole = host.read_sequences(str(path))
        parts = host.read_counted_batches(str(path), [2990, 100, 1], threads=3)
        assert [p.n for p in parts] == [2990, 10, 0]  # fewer at the end of the input, then none
        assert [p.seq(i) for p in parts for i in range(p.n)] == [whole.seq(i) for i in range(whole.n)]


# ---- the output rules on hand-built records ----

M = lambda n: [(n, "M")]


def _rec(flag, tid, pos, nm, cig=None, md="100"):
    return (flag, tid, pos, nm, cig or M(100), md)


def _pairs(mate1, mate2):
    """One record list per mate of each pair: pair i = read i and read n + i."""
    return pm.Records(list(mate1) + list(mate2)), len(mate1)


def test_least_nm_sum_and_the_tie_rules():
    res, n = _pairs([[_rec(0, 0, 1000, 2), _rec(0, 0, 5000, 1), _rec(0, 0, 9000, 1)]],
                    [[_rec(16, 0, 9200, 0), _rec(16, 0, 5200, 0), _rec(16, 0, 1200, 1)]])
    # (1, 1) and (2, 0) both sum to 1: the smaller a wins
    assert pm.choose(res, n, 0, 500) == [(1, 1, 300)]
    res, n = _pairs([[_rec(0, 0, 1000, 1)]], [[_rec(16, 0, 1100, 0), _rec(16, 0, 1150, 0)]])
    assert pm.choose(res, n, 0, 500) == [(0, 0, 200)]  # then the smaller b


def test_the_insert_bounds_are_inclusive():
    res, n = _pairs([[_rec(0, 0, 1000, 0)]], [[_rec(16, 0, 1400, 0, [(50, "M"), (2, "D"), (48, "M")])]])
    assert pm.choose(res, n, 500, 500) == [(0, 0, 500)]  # end0 = 1400 + 50 + 2 + 48
    assert pm.choose(res, n, 501, 600) == [None]
    assert pm.choose(res, n, 0, 499) == [None]


def test_equal_starts_and_mate_2_forward():
    res, n = _pairs([[_rec(16, 0, 1000, 0)]], [[_rec(0, 0, 1000, 0)]])
    assert pm.choose(res, n, 0, 500) == [(0, 0, 100)]
    lines, proper = pm.expected(res, n, 0, 500)
    assert proper == 1 and [l[5] for l in lines] == [-100, 100]  # -insert on the reverse mate's line
    assert [l[2] for l in lines] == [0x1 | 0x2 | 0x40 | 16, 0x1 | 0x2 | 0x80 | 0x20]
    res, n = _pairs([[_rec(16, 0, 999, 0)]], [[_rec(0, 0, 1000, 0)]])
    assert pm.choose(res, n, 0, 500) == [None]  # the forward mate starts behind the reverse one


def test_same_strand_other_sequence_and_asserted_records_are_not_concordant():
    for a, b in ((_rec(0, 0, 1000, 0), _rec(0, 0, 1200, 0)), (_rec(16, 0, 1000, 0), _rec(16, 0, 1200, 0)),
                 (_rec(0, 0, 1000, 0), _rec(16, 1, 1200, 0)), (_rec(0x8000, 0, 1000, 0, [], ""), _rec(16, 0, 1200, 0)),
                 (_rec(0, 0, 1000, 0), _rec(0x8010, 0, 1200, 0, [], ""))):
        res, n = _pairs([[a]], [[b]])
        assert pm.choose(res, n, 0, 500) == [None]
        lines, proper = pm.expected(res, n, 0, 500)
        assert proper == 0 and all(not l[2] & 2 and l[5] == 0 for l in lines)


def test_line_order_flags_and_mate_columns():
    res, n = _pairs([[_rec(0, 0, 100, 2), _rec(0, 1, 7000, 0), _rec(0, 0, 5000, 1)], []],
                    [[_rec(16, 1, 9000, 0), _rec(16, 0, 5100, 0)], [_rec(16, 0, 300, 0)]])
    lines, proper = pm.expected(res, n, 0, 500)
    assert proper == 1
    # pair 0: chosen (2, 1) first in each mate, then the rest in order; pair 1: mate 1 has no record
    assert [l[1] for l in lines] == [2, 0, 1, 4, 3, 5]
    assert [l[2] for l in lines] == [0x43 | 0x20, 0x41 | 256 | 0x20, 0x41 | 256 | 0x20, 0x83 | 16, 0x81 | 16 | 256, 0x81 | 16 | 0x8]
    assert [l[3] for l in lines] == [0, 0, 0, 0, 0, None]
    assert [l[4] for l in lines] == [5100] * 3 + [5000] * 2 + [None]
    assert [l[5] for l in lines] == [200, 0, 0, -200, 0, 0]
    text = pm.sam_lines(res, n, ["chrA", "chrB"], [b"A" * 100] * 4, ["p0", "p1", "p0", "p1"], ["I" * 100] * 4)
    cols = [l.split("\t") for l in text.splitlines()]
    assert [c[6:9] for c in cols] == [["=", "5101", "200"], ["=", "5101", "0"], ["chrA", "5101", "0"],
                                      ["=", "5001", "-200"], ["chrA", "5001", "0"], ["*", "0", "0"]]
    assert [c[9] != "*" for c in cols] == [True, False, False, True, False, True]
    arrays = pm.pair_arrays(res, n, 0, 500)
    assert list(arrays["rec_begin"]) == [0, 3, 5, 5, 6]


def test_strip_mate_suffix():
    assert [pm.strip_mate_suffix(x) for x in ("a/1", "a/2", "a/3", "a", "/1", "a1")] == ["a", "a", "a/3", "a", "", "a1"]
