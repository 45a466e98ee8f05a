"""The MAPQ rule of FEM map --mapq (tests/mapq_model.py) on hand-built records, and the option's CPU-side handling."""
from tests import mapq_model as mq
from tests import pair_model as pm
from tests.harness import run_fem


def rec(nm, pos=1000, flag=0, tid=0, L=100):
    return (flag, tid, pos, nm, [(L, "M")], str(L))


def se(*nms):
    return pm.Records([[rec(x, 1000 + 5000 * k) for k, x in enumerate(nms)]])


def test_worked_values():
    for nms, want in [((0,), 60), ((3,), 20), ((2,), 40), ((0, 1), 20), ((0, 2, 2, 2, 2), 34), ((1, 1, 2), 0),
                      ((0,) + (1,) * 1024, 0)]:
        assert mq.single_end(se(*nms), 3) == [want] + [0] * (len(nms) - 1), nms


def test_the_formula():
    assert [mq.Q(g, 1) for g in (1, 2, 3, 4)] == [20, 40, 60, 60]
    assert [mq.Q(1, c) for c in (1, 2, 3, 4, 7, 8, 64, 128)] == [20, 17, 17, 14, 14, 11, 2, 0]
    assert mq.Q(0, 1) == 0 and mq.Q(3, 2 ** 40) == 0 and mq.Q(4, 2 ** 31) == 0 and mq.Q(5, 2 ** 10) == 60


def test_single_end_branches():
    assert mq.q_se([2, 2], 3) == 0 and mq.q_se([0, 0, 1], 7) == 0          # ties
    assert [mq.q_se([0, g], 7) for g in (1, 2, 3, 4)] == [20, 40, 60, 60]  # gaps 1-4
    assert mq.q_se([0, 3, 3], 7) == 57 and mq.q_se([0, 3, 3, 3, 3], 7) == 54  # the c2 penalty
    assert mq.q_se([0, 2, 3, 3], 7) == 40                                  # only the least NM above d1 counts
    assert mq.q_se([3], 3) == 20 and mq.q_se([7], 7) == 20 and mq.q_se([0], 0) == 20  # d1 = e
    assert mq.q_se([1], 3) == 60 and mq.q_se([1], 2) == 40
    assert mq.q_se([], 3) == 0


def _pair(a, b):
    return pm.Records([a, b])


def test_worked_pair():
    # mate A: two NM-0 records 10 kb apart; mate B: one NM-0 record, concordant with A's first only (X = 500)
    res = _pair([rec(0, 1000), rec(0, 11000)], [rec(0, 1300, 16)])
    assert mq.paired(res, 1, 3, 0, 500) == [40, 0, 60]
    assert mq.single_end(res, 3) == [0, 0, 60]


def test_pair_branches():
    # a proper pair alone: qp = 60, each mate's own value rises by at most 40
    res = _pair([rec(2, 1000)], [rec(1, 1300, 16)])
    assert mq.paired(res, 1, 3, 0, 500) == [60, 60]
    res = _pair([rec(3, 1000)], [rec(3, 1300, 16)])
    assert mq.paired(res, 1, 3, 0, 500) == [60, 60]  # q_se 20 each, qp 60: min(60, 60) = 60
    # two concordant combinations at one sum: qp 0, the mates keep their own values
    res = _pair([rec(0, 1000)], [rec(0, 1300, 16), rec(0, 1350, 16)])
    assert mq.paired(res, 1, 3, 0, 500) == [60, 0, 0]
    # the next concordant sum one edit above, twice: qp = Q(1, 2) = 17
    res = _pair([rec(0, 1000), rec(0, 9000)], [rec(0, 1300, 16), rec(1, 1320, 16), rec(1, 9300, 16)])
    assert mq.paired(res, 1, 3, 0, 500) == [17, 0, 17, 0, 0]
    # a chosen record above its mate's best single-end hit: q_x = 0, only the pair speaks for it
    res = _pair([rec(0, 1000), rec(1, 20000)], [rec(0, 20300, 16)])
    assert mq.paired(res, 1, 3, 0, 500) == [40, 0, 60]  # chosen (a=1, b=0): A's q_x = 0, qp = 60 -> 40
    # not a proper pair (same strand): each mate's primary line its own value
    res = _pair([rec(0, 1000), rec(1, 5000)], [rec(0, 1300)])
    assert mq.paired(res, 1, 3, 0, 500) == [20, 0, 60]
    # secondary lines are 0 and a mate without records has no line
    res = _pair([rec(1, 1000), rec(2, 1200, 16), rec(2, 8000)], [])
    assert mq.paired(res, 1, 3, 0, 500) == [17, 0, 0]


def test_rescued_mate():
    se_res = _pair([rec(0, 1000), rec(0, 30000)], [])
    rescued = _pair([rec(0, 1000), rec(0, 30000)], [rec(2, 1300, 16)])
    assert mq.paired(se_res, 1, 3, 0, 500, res=rescued, rescued={1}) == [40, 0, 40]  # q_x 0 for both: A tied, B from a window
    se_res = _pair([rec(0, 1000)], [])
    rescued = _pair([rec(0, 1000)], [rec(5, 1300, 16)])
    assert mq.paired(se_res, 1, 3, 0, 500, res=rescued, rescued={1}) == [60, 40]


def _line(name, flag, pos, nm, cigar="100M"):
    return "\t".join([name, str(flag), "s0", str(pos), "255", cigar, "*", "0", "0", "*", "*", "NM:i:%d" % nm, "MD:Z:100"])


def test_from_sam_agrees_with_the_records():
    se_text = "\n".join([_line("r1", 0, 1001, 0), _line("r1", 256, 5001, 1), _line("r2", 16, 3001, 1), _line("r3", 0, 9, 2),
                         _line("r3", 272, 99, 2)]) + "\n"
    assert mq.from_sam(se_text, 3) == [20, 0, 60, 0, 0]
    # the worked pair as FEM writes it: mate 1's lines, then mate 2's, the chosen record first
    p = "\n".join([_line("p", 0x63, 1001, 0), _line("p", 0x161, 11001, 0), _line("p", 0x93, 1301, 0)]) + "\n"
    assert mq.from_sam(p, 3, True, 0, 500) == [40, 0, 60]
    # not proper, mate 2 without records
    p = "\n".join([_line("q", 0x49, 1001, 1)]) + "\n"
    assert mq.from_sam(p, 3, True, 0, 500) == [60]
    assert mq.column5(mq.with_mapq(p, [7])) == [7]


def _fem(*args, env=None):
    return run_fem(*args, env=env)


def test_cli_lists_and_refuses_mapq(tmp_path):
    import __graft_entry__ as g
    g.build()
    r = _fem("map", "-h")
    assert r.returncode == 0 and b"--mapq" in r.stderr
    args = ["map", "--mapq", "--ref", str(tmp_path / "none.fa"), "--index", str(tmp_path / "none.idx"), "--read1",
            str(tmp_path / "none.fq"), "-o", str(tmp_path / "out.sam")]
    for v in ("FEM_HOST_TAIL", "FEM_HOST_FORMAT"):
        r = _fem(*args, env={v: "1"})
        assert r.returncode == 1, r.stderr
        assert b"--mapq is not supported with " + v.encode() + b"=1" in r.stderr
        assert b"Loaded index" not in r.stderr
