"""Mate rescue, the parts that need no GPU: the oracle's banded Myers and traceback at the rescue's edit bounds (8..15)
against the Python matrix models, the rule of tests/rescue_model.py on hand-built cases, and FEM map's --rescue checks."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import pair_model as pm
from tests import rescue_model as rm
from tests import util
from tests.cases import Asserted, banded_dp, model_align
from tests.harness import run_fem


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


# ---- the oracle at E = 8 .. 15 (2E + 1 <= 32: one 32-bit word) ----

@pytest.mark.parametrize("E", list(range(8, 16)))
def test_myers32_and_traceback_at_rescue_bounds(E):
    rng = np.random.default_rng(300 + E)
    n_acc = n_indel = 0
    for trial in range(40):
        L = int(rng.integers(40, 160))
        ref = util.rand_seq(rng, L + 4 * E + 8)
        shift = int(rng.integers(0, 2 * E + 1))
        read = util.mutate(rng, ref[shift:shift + L + E], int(rng.integers(0, E + 3)))[:L]
        if len(read) < L:
            read += util.rand_seq(rng, L - len(read))
        ed, end = fo.banded_ed32(E, ref, read)
        m_ed, m_end = banded_dp(E, ref, read)
        assert ed == m_ed and (ed > E or end == m_end), (E, trial)
        if ed > E:
            continue
        o = fo.align(E, ref, read, ed, end)
        try:
            m_start, m_cig, m_md = model_align(E, ref, read, ed, end)
        except Asserted:
            assert o[0] < 0
            continue
        assert o == (m_start, "".join("%d%s" % (n, op) for op, n in m_cig), m_md), (E, trial)
        n_acc += 1
        n_indel += any(op != "M" for op, _ in m_cig)
    assert n_acc >= 20 and n_indel >= 5


# ---- the rule on hand-built cases ----

def _case(seq, anchors, b, E=4, I=0, X=500, b_first=False):
    """One pair on one sequence: mate 1 has `anchors` (flag, pos0, nm, cigar), mate 2 (read b) none (swapped: b_first)."""
    recs = [(fl, 0, p, nm, cig, "") for fl, p, nm, cig in anchors]
    per_read = [[], recs] if b_first else [recs, []]
    reads = [b, b"A" * 100] if b_first else [b"A" * 100, b]
    res = pm.Records(per_read)
    return rm.rescue(res, 1, reads, [seq], E, I, X)


def _seq(seed=1, n=5000):
    return util.rand_seq(np.random.default_rng(seed), n)


def test_window_bounds_are_inclusive_on_both_strands():
    s = _seq()
    # anchor forward at 1000: B reverse-complemented, hi = 1000 + 500 - 100
    ext, kept, _ = _case(s, [(0, 1000, 0, [(100, "M")])], util.revcomp(s[1400:1500]))
    assert [(k["record"][0], k["record"][2], k["record"][3], k["record"][4]) for k in kept.values()] == [(16, 1400, 0, [(100, "M")])]
    _, kept, _ = _case(s, [(0, 1000, 0, [(100, "M")])], util.revcomp(s[1401:1501]))
    assert not any(k["record"][3] == 0 for k in kept.values())
    # anchor reverse at 2000 (end 2100): B forward, lo = 2100 - 500; I = 50: hi = min(2000, 2100 - 50)
    _, kept, _ = _case(s, [(16, 2000, 0, [(100, "M")])], s[1600:1700], I=50, b_first=True)
    assert [(k["b_read"], k["record"][0], k["record"][2]) for k in kept.values()] == [(0, 0, 1600)]
    _, kept, _ = _case(s, [(16, 2000, 0, [(100, "M")])], s[1599:1699], I=50, b_first=True)
    assert not any(k["record"][3] == 0 for k in kept.values())
    _, kept, _ = _case(s, [(16, 2000, 0, [(100, "M")])], s[2000:2100], I=50, b_first=True)  # hi = min(2000, 2050)
    assert [k["record"][2] for k in kept.values()] == [2000]
    _, kept, _ = _case(s, [(16, 2000, 0, [(100, "M")])], s[2001:2101], I=50, b_first=True)
    assert not any(k["record"][3] == 0 for k in kept.values())


def test_tiles_cut_at_the_sequence_end():
    s = _seq(2, 3000)
    L, E = 100, 4
    # anchor forward at 2500: lo = 2500, tiles 2500, 2509, ...; B at the very end (2900): its tile needs 2900 + L + 2E bases
    _, kept, _ = _case(s, [(0, 2500, 0, [(100, "M")])], util.revcomp(s[2900:3000]), E=E)
    assert not any(k["record"][2] == 2900 for k in kept.values())
    # 2E + 1 bases further in: found
    _, kept, _ = _case(s, [(0, 2500, 0, [(100, "M")])], util.revcomp(s[2891:2991]), E=E)
    assert [k["record"][2] for k in kept.values()] == [2891]


def test_eight_anchors_at_most_and_broken_records_skipped():
    s = _seq(3)
    far = [(0, 100 + 7 * i, 1, [(100, "M")]) for i in range(8)]
    real = (0, 3000, 0, [(100, "M")])
    b = util.revcomp(s[3200:3300])
    _, kept, _ = _case(s, far[:7] + [real], b)
    assert [k["a"] for k in kept.values()] == [7]
    _, kept, _ = _case(s, far + [real], b)  # the ninth record is no anchor
    assert not kept
    _, kept, _ = _case(s, [(0x8000, 3000, 0, [])], b)
    assert not kept
    _, kept, _ = _case(s, far[:3] + [(0x8000, 0, 0, [])] + far[3:7] + [real], b)  # a broken one counts to the eight
    assert not kept


def test_ties_across_anchors_and_within_a_tile():
    s = _seq(4)
    b = util.revcomp(s[3200:3300])
    _, kept, _ = _case(s, [(0, 3000, 0, [(100, "M")]), (0, 3000, 0, [(100, "M")])], b)
    assert [k["a"] for k in kept.values()] == [0]
    _, kept, _ = _case(s, [(0, 3000, 2, [(100, "M")]), (0, 3000, 0, [(100, "M")])], b)
    assert [k["a"] for k in kept.values()] == [1]
    # a tandem repeat: every other offset matches; the first strict minimum and the least pos0 win
    t = s[:3000] + b"AC" * 150 + s[3300:]
    _, kept, _ = _case(t, [(0, 2800, 0, [(100, "M")])], util.revcomp(b"AC" * 50), E=4)
    (k,) = kept.values()
    assert k["record"][2] == 3000 and k["record"][3] == 0


def test_no_rescue_when_both_mates_have_records():
    s = _seq(5)
    recs = [[(0, 0, 1000, 0, [(100, "M")], "100")], [(16, 0, 4000, 0, [(100, "M")], "100")]]
    res = pm.Records(recs)
    ext, kept, traced = rm.rescue(res, 1, [s[1000:1100], util.revcomp(s[1300:1400])], [s], 8)
    assert not kept and not traced


def test_a_mate_of_length_0_is_not_searched():
    s = _seq(7)
    for anchor, b_first in (((0, 1000, 0, [(100, "M")]), False), ((16, 2000, 0, [(100, "M")]), True)):
        ext, kept, traced = _case(s, [anchor], b"", b_first=b_first)
        assert not kept and not traced
        assert ext.rec_off.tolist() == ([0, 0, 1] if b_first else [0, 1, 1])  # the pair stays as it was


def test_reverse_mate_pushed_past_x_is_dropped():
    s = _seq(6)
    assert s[1500:1501] == b"G"
    # anchor forward at 1000, X = 500: B reverse, its last base (as searched) an extra A.  The search ends it at 1499 (pos0
    # 1400 = hi); the traceback folds that end insertion into the M run: 100M from 1401, an insert of 501 > X: dropped
    b = util.revcomp(s[1401:1500] + b"A")
    ext, kept, traced = _case(s, [(0, 1000, 0, [(100, "M")])], b, E=4)
    assert not kept
    (t,) = traced.values()
    assert t["hit"][:2] == (1, 1400) and t["record"][2] == 1401 and t["record"][4] == [(100, "M")]
    assert ext.rec_off.tolist() == [0, 1, 1]  # the pair stays as it was
    # with X = 501: kept
    _, kept, _ = _case(s, [(0, 1000, 0, [(100, "M")])], b, E=4, X=501)
    assert [(k["record"][2], k["record"][3]) for k in kept.values()] == [(1401, 1)]


def test_lower_case_window_gives_an_md_of_every_column():
    # a soft-masked window: codes match (the search), characters do not (the walk, MD): the record is kept with an MD that
    # names every reference base, far more than a walk of E errors on canonical characters needs
    s = _seq(7)
    s = s[:1300] + s[1300:1500].lower() + s[1500:]
    t = bytearray(s[1400:1500].upper())
    t[99] = ord("A") if t[99] != ord("A") else ord("C")  # one substitution at the read's 3' end (as searched)
    _, kept, _ = _case(s, [(0, 1000, 0, [(100, "M")])], util.revcomp(bytes(t)), E=4)
    (k,) = kept.values()
    assert k["record"][2:5] == (1400, 1, [(100, "M")]) and len(k["record"][5]) == 100 > 8 * 4 + 64


# ---- FEM map --rescue ----

def run(*args):
    return run_fem(*args, text=True)


def test_usage_lists_rescue():
    assert "--rescue" in run("map", "-h").stderr


@pytest.mark.parametrize("extra,msg", [
    (["--rescue", "8"], "--rescue needs read pairs (--read2)."),
    (["--read2", "r2.fq", "--rescue", "16"], "Wrong rescue error threshold (0-15)."),
    (["--read2", "r2.fq", "--rescue", "-1"], "Wrong rescue error threshold (0-15)."),
    (["--read2", "r2.fq", "--rescue", "x"], "Wrong rescue error threshold (0-15)."),
    (["--read2", "r2.fq", "--rescue", "8", "-I", "10", "-X", "65547"], "--rescue searches insert size ranges of at most 65536."),
])
def test_rescue_refusals(tmp_path, extra, msg):
    args = ["map", "-e", "3", "--ref", str(tmp_path / "x.fa"), "--index", str(tmp_path / "x.idx"), "--read1", str(tmp_path / "r1.fq"),
            "-o", str(tmp_path / "o.sam")] + [str(tmp_path / a) if a == "r2.fq" else a for a in extra]
    r = run(*args)
    assert r.returncode == 1 and msg in r.stderr
