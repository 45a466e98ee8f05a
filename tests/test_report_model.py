"""The model of the line filter (tests/report_model.py) on hand-built records: every row of the rule of include/fem_hip.h
(fem_dev_set_report) at least once; on the oracle, without a GPU, that the case generators of tests/cases.py give what
their cases need; and the argument errors of FEM map --strata / --max-hits."""
from tests import cases
from tests import pair_model as pm
from tests import report_model as rp
from tests import unmapped_model as um
from tests.harness import run_fem

SEQS = ["chrA", "chrB"]


def _rec(pos, nm, flag=0):
    return (flag, 0, pos, nm, [(5, "M")], "5")


def _pos(text):
    return [int(l.split(b"\t")[3]) - 1 for l in text.splitlines()]


def _single(per_read, **kw):
    n = len(per_read)
    res = pm.Records([[_rec(p, nm, f | (256 if t else 0)) for t, (p, nm, f) in enumerate(r)] for r in per_read])
    text = um.single_end(res, SEQS, [b"ACGTA"] * n, ["r%d" % i for i in range(n)], ["IIIII"] * n, e=kw.pop("e", None))
    if not kw.pop("unmapped", False):
        text = um.without_unmapped(text)[0]
    return text, rp.apply(text, **kw)


def test_keep():
    assert rp.keep([3]) == [True] and rp.keep([3], 0, 1) == [True]
    assert rp.keep([0, 0, 1, 1, 2], max_hits=1) == [True, False, False, False, False]
    assert rp.keep([0, 0, 1, 1, 2], max_hits=5) == [True] * 5
    assert rp.keep([0, 0, 1, 1, 2], max_hits=4) == [True] * 4 + [False]
    assert rp.keep([0, 0, 1, 1, 2], strata=0) == [True, True, False, False, False]
    assert rp.keep([0, 0, 1, 1, 2], strata=1) == [True] * 4 + [False]
    assert rp.keep([0, 0, 1, 1, 2], strata=15, max_hits=2 ** 31 - 1) == [True] * 5
    # the primary line outside the best stratum: kept, and the others are measured from d, not from it
    assert rp.keep([2, 0, 1, 2, 0], strata=0) == [True, True, False, False, True]
    assert rp.keep([2, 0, 1, 2, 0], strata=1) == [True, True, True, False, True]
    # S and N together: N counts the kept lines only, the primary line among them
    assert rp.keep([2, 3, 0, 1, 0, 0], strata=0, max_hits=3) == [True, False, True, False, True, False]
    assert rp.keep([1, 0, 2, 0], strata=0, max_hits=1) == [True, False, False, False]


def test_single_end_rows():
    # read 0: one line; read 1: five lines in two strata and a third; read 2: none; read 3: two lines, the second one asserted (0x8000)
    per_read = [[(10, 2, 0)], [(20, 0, 0), (21, 0, 16), (22, 1, 0), (23, 1, 0), (24, 3, 16)], [], [(40, 1, 0), (41, 1, 0x8000)]]
    text, (got, dropped) = _single(per_read, max_hits=1)
    assert _pos(got) == [10, 20, 40] and dropped == 5
    # a kept line is the line it was: byte for byte
    assert all(l in text.splitlines() for l in got.splitlines())
    _, (got, dropped) = _single(per_read, max_hits=5)  # N = the line count
    assert _pos(got) == [10, 20, 21, 22, 23, 24, 40, 41] and dropped == 0
    _, (got, dropped) = _single(per_read, max_hits=4)  # ... and the count - 1
    assert _pos(got) == [10, 20, 21, 22, 23, 40, 41] and dropped == 1
    _, (got, dropped) = _single(per_read, strata=0)  # (a 0x8000 record counts like any other)
    assert _pos(got) == [10, 20, 21, 40, 41] and dropped == 3
    _, (got, dropped) = _single(per_read, strata=1, max_hits=3)
    assert _pos(got) == [10, 20, 21, 22, 40, 41] and dropped == 2
    _, (got, dropped) = _single(per_read, strata=2)
    assert _pos(got) == [10, 20, 21, 22, 23, 40, 41] and dropped == 1
    # both off, and the widest filter: the text itself
    assert rp.apply(text) == (text, 0) and rp.apply(text, 15, 2 ** 31 - 1) == (text, 0)
    # an unmapped read's line is a slot of its own and stays; MAPQ is what it was
    text, (got, dropped) = _single(per_read, unmapped=True, e=3, strata=0, max_hits=1)
    f = [l.split(b"\t") for l in got.splitlines()]
    assert [x[0] for x in f] == [b"r0", b"r1", b"r2", b"r3"] and int(f[2][1]) == 4 and dropped == 5
    assert [x[4] for x in f] == [x[4] for x in (l.split(b"\t") for l in text.splitlines()) if not int(x[1]) & 256]


def test_pair_rows():
    # pair 0: mate 1 has records at NM 0 (far away), 2 (concordant with mate 2) and 1 (far away): the chosen one has NM 2
    # pair 1: only mate 2 maps (three lines); pair 2: neither
    m = lambda flag, pos, nm: (flag, 0, pos, nm, [(5, "M")], "5")
    res = pm.Records([[m(0, 5000, 0), m(256, 100, 2), m(256, 9000, 1)], [], [],
                      [m(16, 300, 0), m(16 | 256, 7000, 0)], [m(0, 400, 1), m(256, 500, 1), m(256, 600, 2)], []])
    reads, names, quals = [b"ACGTA"] * 6, ["p0", "p1", "p2"] * 2, ["IIIII"] * 6
    full = um.paired(res, 3, SEQS, reads, names, quals, e=3)
    assert _pos(full)[:5] == [100, 5000, 9000, 300, 7000] and int(full.split(b"\t")[1]) & 2
    assert [len(s) for s in rp.slots(full)] == [3, 2, 1, 3, 1, 1]
    # S = 0: the chosen record stays although its NM is 2; d is 0, so of the others only the NM 0 line stays
    got, dropped = rp.apply(full, strata=0)
    assert _pos(got)[:4] == [100, 5000, 300, 7000] and dropped == 2
    assert rp.keep([2, 0, 1], strata=1) == [True, True, True]
    # N = 1: one line per mapped mate; the unmapped mates' lines stay, placed at a first line that is there
    got, dropped = rp.apply(full, max_hits=1)
    f = [l.split(b"\t") for l in got.splitlines()]
    assert [(x[0], int(x[3])) for x in f] == [(b"p0", 101), (b"p0", 301), (b"p1", 401), (b"p1", 401), (b"p2", 0), (b"p2", 0)]
    assert dropped == 5 and f[3][6:8] == [b"=", b"401"]
    # without the unmapped reads' lines: the same rule on the default text
    plain = um.without_unmapped(full, True)[0]
    got, dropped = rp.paired(res, 3, SEQS, reads, names, quals, e=3, unmapped=False, strata=0, max_hits=2)
    assert got == rp.apply(plain, 0, 2)[0] and _pos(got) == [100, 5000, 300, 7000, 400, 500] and dropped == 2


# ---- the generators of the GPU cases meet their bounds (oracle and rescue model, no GPU) ----

def test_generated_single_end_cases():
    for case in cases.REPORT_SINGLE_CASES:
        cases.check_report_single_case(cases.report_single_case(*case))


def test_generated_pair_cases():
    assert any(c[4] is None for c in cases.REPORT_PAIR_CASES) and any(c[4] is not None for c in cases.REPORT_PAIR_CASES)
    for case in cases.REPORT_PAIR_CASES:
        cases.check_report_pair_case(cases.report_pair_case(*case))


# ---- FEM map --strata / --max-hits: the argument errors ----

def _run(*args, env=None):
    return run_fem("map", "--ref", "a", "--index", "b", "--read1", "c", "-o", "d", *args, env=env)


def test_cli_argument_errors():
    import __graft_entry__ as g
    g.build()
    for args, message in ((["--max-hits", "0"], b"Wrong hit limit (>= 1)."), (["--max-hits", "x"], b"Wrong hit limit (>= 1)."),
                          (["--max-hits", "2147483648"], b"Wrong hit limit (>= 1)."),
                          (["--strata", "16"], b"Wrong number of strata (0-15)."), (["--strata", "x"], b"Wrong number of strata (0-15)."),
                          (["--strata", "-1"], b"Wrong number of strata (0-15).")):
        r = _run(*args)
        assert r.returncode == 1 and message in r.stderr and b"--max-hits INT" in r.stderr and b"--strata INT" in r.stderr, args
    for v in ("FEM_HOST_FORMAT", "FEM_HOST_TAIL"):
        for args in (["--strata", "0"], ["--max-hits", "2"]):
            r = _run(*args, env={v: "1"})
            assert r.returncode != 0 and ("--strata and --max-hits are not supported with %s=1" % v).encode() in r.stderr
