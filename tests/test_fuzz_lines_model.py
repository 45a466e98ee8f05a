"""The model side of tests/fuzz_lines.py, without a GPU, on the exact (seed, trial) list of tests/test_gpu_fuzz_lines.py: draw()
is a function of (seed, trial) alone; the slice reaches the places where the kernels of fem_tail.hip go wrong (wave paths, ties,
inserts on a bound, lines out of NM order, the filter on 0x8000 records, ...); and an off-by-one in any parameter of the rule
changes the expected text of some trial, so that a device with it could not pass.  The figures are conditions on the committed
slice: a seed list that misses one is changed, never the condition."""
import functools

import numpy as np
import pytest

from tests import fuzz_lines as fl
from tests import pair_model as pm
from tests import report_model as rp
from tests import rescue_model as rm

K_ALONE = 32  # fem_tail.hip, kPairAlone / kMapqAlone / kReportAlone: more combinations or lines are their wave's
MIN_TRIALS = 3
MIN_SENSITIVE = 2


@functools.lru_cache(maxsize=None)
def trials():
    """[(trial, its expected result)] of the slice, drawn once."""
    out = []
    for seed, k, force in fl.slice_trials():
        t = fl.draw(np.random.default_rng([seed, k]), force)
        out.append((t, fl.expected(t, full=False)))
    return out


def test_draw_depends_on_seed_and_trial_alone():
    for (seed, k, force), (t, _) in list(zip(fl.slice_trials(), trials()))[::5]:
        again = fl.draw(np.random.default_rng([seed, k]), force)
        assert fl.fingerprint(again) == fl.fingerprint(t), (seed, k)
    a, b = (fl.draw(np.random.default_rng([11, k])) for k in (0, 1))
    assert fl.fingerprint(a) != fl.fingerprint(b)


def test_the_slice_has_its_four_kinds_of_case():
    by_id = {c[0]: [t for (t, _), (seed, _, _) in zip(trials(), fl.slice_trials()) if seed == c[1]] for c in fl.SLICE}
    assert len(by_id) == 4 and all(len(v) == c[2] for v, c in zip(by_id.values(), fl.SLICE))
    assert sum(not t.paired for t in by_id["single-end-heavy"]) >= len(by_id["single-end-heavy"]) // 2
    assert all(t.copies == 80 for t in by_id["copies-80"]) and all(t.e == 7 for t in by_id["e-7"])
    assert sum(t.cli and t.paired for t in by_id["command-line"]) == 1
    for t, _ in trials():  # the drawn ranges
        assert 37 + 12 * t.e <= min(t.L, t.L2) and max(t.L, t.L2) <= 260 and 0 <= t.E <= 15 and 0 <= t.I <= t.X
        assert not t.rescue or t.X - t.I <= 65536
        assert all(1 <= len(x) <= 254 for x in t.rnames) and (t.rg is None or 1 <= len(t.rg) <= 255)
        assert not t.packed or (t.L == t.L2 and all(len(r) == t.L for r in t.reads))


def features(t, w):
    """Which of the places named above trial t reaches (a set of names)."""
    out = set()
    if int(t.se.rec_off[-1]) == 0:
        out.add("nothing maps")
    lines = [l.split(b"\t") for l in w.plain.split(b"\n") if l]
    if t.paired:
        n, ext = t.n, w.ext
        cnt = np.diff(ext.rec_off.astype(np.int64))
        if any(cnt[i] * cnt[n + i] > K_ALONE for i in range(n)):
            out.add("a pair with more than 32 combinations")
        kept_kinds = {k for k, _ in w.kinds.values()}
        out |= {"a kept kind-%d rescue" % k for k in kept_kinds}
        if any(r.get("tie") for r in w.traced.values()):
            out.add("a kind-2 rescue with equal sums in both directions")
        if any(not r["kept"] for r in w.traced.values()):
            out.add("a rescue traced but not kept")
        ins = fl.occurring_inserts(ext, n, t.I, t.X)
        if t.X in ins:
            out.add("ins == X")
        if t.I > 0 and t.I in ins:
            out.add("ins == I > 0")
        chosen = pm.choose(ext, n, t.I, t.X)
        if any(c is not None and (c[0] > 0 or c[1] > 0) for c in chosen):
            out.add("a chosen record that is not its mate's first")
        for recs in pm.line_order(ext, n, chosen):
            nms = [int(ext.r_nm[j]) for j in recs]
            if nms != sorted(nms):
                out.add("a mate whose lines are not in NM order")
        if any(int(f[1]) & 4 and f[2] != b"*" for f in lines):
            out.add("a placed unmapped mate")
        if any(int(f[1]) & 4 and int(f[1]) & 8 for f in lines):
            out.add("a pair with both mates unmapped")
    else:
        cnt = np.diff(t.se.rec_off.astype(np.int64))
    if cnt.max(initial=0) > K_ALONE:
        out.add("a mate with more than 32 lines")
    if t.strata is not None or t.max_hits is not None:
        whole = fl.expected(t, full=False, strata=None, max_hits=None).plain
        for slot in rp.slots(whole):
            if int(slot[0].split(b"\t", 2)[1]) & 4:
                continue
            nms = [rp.line_nm(l) for l in slot]
            if all(rp.keep(nms, t.strata, t.max_hits)):
                continue
            if any(l.split(b"\t")[5] == b"*" for l in slot):
                out.add("a 0x8000 record among a filtered slot's lines")
            if t.strata is not None and t.max_hits is not None:
                by_strata = [k for k in rp.keep(nms, t.strata, None)]
                if not all(by_strata) and sum(by_strata) > t.max_hits:
                    out.add("a slot cut by max_hits and by strata")
    return out


COVERAGE = ["a pair with more than 32 combinations", "a mate with more than 32 lines", "a kept kind-2 rescue", "a kept kind-1 rescue",
            "a kind-2 rescue with equal sums in both directions", "a rescue traced but not kept", "ins == X", "ins == I > 0",
            "a chosen record that is not its mate's first", "a mate whose lines are not in NM order", "a placed unmapped mate",
            "a pair with both mates unmapped", "a 0x8000 record among a filtered slot's lines", "a slot cut by max_hits and by strata"]


@functools.lru_cache(maxsize=None)
def found():
    return [features(t, w) for t, w in trials()]


@pytest.mark.parametrize("what", COVERAGE)
def test_coverage(what):
    hits = sum(what in f for f in found())
    assert hits >= MIN_TRIALS, "%s: in %d of %d trials" % (what, hits, len(found()))


def test_most_trials_map_something():
    assert 10 * sum("nothing maps" in f for f in found()) <= len(found())


def _anchors(n):
    def text(t):
        old = rm.ANCHORS
        rm.ANCHORS = n
        try:
            return fl.expected(t, full=False).text
        finally:
            rm.ANCHORS = old
    return text


class _LastOfTheLeast:
    """numpy with an argmin that takes the last of equal minima: pair_model.choose with ties to the larger index in B."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argmin(s):
        return len(s) - 1 - int(np.argmin(s[::-1]))


def _last_b(t):
    t.__dict__.pop("_rescued", None)  # (the kind-2 candidates do not depend on the tie, but nothing patched is kept)
    pm.np = _LastOfTheLeast()
    try:
        return fl.expected(t, full=False).text
    finally:
        pm.np = np
        t.__dict__.pop("_rescued", None)


# the parameter a device might have one off: where it is defined for a trial, the expected text with it
PERTURBATIONS = {
    "X - 1": (lambda t: t.paired and t.X - 1 >= t.I, lambda t: fl.expected(t, full=False, X=t.X - 1).text),
    "I + 1": (lambda t: t.paired and t.I + 1 <= t.X, lambda t: fl.expected(t, full=False, I=t.I + 1).text),
    "E - 1": (lambda t: t.paired and t.rescue and t.E >= 1, lambda t: fl.expected(t, full=False, E=t.E - 1).text),
    "S - 1": (lambda t: t.strata is not None and t.strata >= 1, lambda t: fl.expected(t, full=False, strata=t.strata - 1).text),
    "S + 1": (lambda t: t.strata is not None and t.strata <= 14, lambda t: fl.expected(t, full=False, strata=t.strata + 1).text),
    "N - 1": (lambda t: t.max_hits is not None and t.max_hits >= 2, lambda t: fl.expected(t, full=False, max_hits=t.max_hits - 1).text),
    "N + 1": (lambda t: t.max_hits is not None and t.max_hits < (1 << 31) - 1, lambda t: fl.expected(t, full=False, max_hits=t.max_hits + 1).text),
    "MAPQ at e + 1": (lambda t: t.mapq, lambda t: fl.expected(t, full=False, mapq_e=t.e + 1).text),
    "7 anchors": (lambda t: t.paired and t.rescue, _anchors(7)),
    "the last b at equal sums": (lambda t: t.paired, _last_b),
}


@pytest.mark.parametrize("what", sorted(PERTURBATIONS))
def test_sensitivity(what):
    defined, text = PERTURBATIONS[what]
    seen = sum(1 for t, w in trials() if defined(t) and text(t) != w.text)
    assert seen >= MIN_SENSITIVE, "%s changes the expected text of %d trials" % (what, seen)
    assert rm.ANCHORS == 8
