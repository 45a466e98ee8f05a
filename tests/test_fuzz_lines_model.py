"""The model side of tests/fuzz_lines.py, without a GPU, on the exact (seed, trial) list of tests/test_gpu_fuzz_lines.py: draw()
is a function of (seed, trial) alone; the slice reaches the places where the kernels of fem_tail.hip go wrong (wave paths, ties,
inserts on a bound, lines out of NM order, the filter on 0x8000 records, rescues of either kind under RF and FF, turned lines with
IUPAC letters, folds of 1, 31-33 and 64 or more entries, the byte budget met exactly, the mate tags of rescued, placed and
untraced mates, the refusal of host qualities, ...); and an off-by-one in any parameter of the rule, or a strand taken from the
wrong one of the real and the virtual world, changes the expected text of some trial, so that a device with it could not pass.
The figures are conditions on the committed slice: a seed list that misses one is changed, never the condition.

A perturbation recomputes only the stages behind the one it touches (fuzz_lines keeps a trial's records and its text up to
real_text per parameter set; lines_behind makes the rest).  The file took 14 s before the orientation, the mate tags, --sam-seq
and --xa were drawn (48 trials, 24 conditions) and takes 30 s with them (72 trials, 63 conditions), on the same machine."""
import functools
import types

import numpy as np
import pytest

from tests import fuzz_lines as fl
from tests import mate_tags_model as mt
from tests import orient_model as om
from tests import pair_model as pm
from tests import report_model as rp
from tests import rescue_model as rm
from tests import sam_seq_model as ss
from tests import xa_model as xm

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
    assert len(by_id) == len(fl.SLICE) >= 4 and all(len(v) == c[2] for v, c in zip(by_id.values(), fl.SLICE))
    assert sum(not t.paired for t in by_id["single-end-heavy"]) >= len(by_id["single-end-heavy"]) // 2
    assert all(t.copies == 80 for t in by_id["copies-80"]) and all(t.e == 7 for t in by_id["e-7"])
    assert sum(t.cli and t.paired for t in by_id["command-line"]) == 1
    for t, _ in trials():  # the drawn ranges
        assert 37 + 12 * t.e <= min(t.L, t.L2) and max(t.L, t.L2) <= 260 and 0 <= t.E <= 15 and 0 <= t.I <= t.X
        assert not t.rescue or t.X - t.I <= 65536
        assert all(1 <= len(x) <= 254 for x in t.rnames) and (t.rg is None or 1 <= len(t.rg) <= 255)
        assert not t.packed or (t.L == t.L2 and all(len(r) == t.L for r in t.reads))
        assert t.orientation in (0, 1, 2) and (t.xa is None or 1 <= t.xa <= 2 ** 31 - 1) and t.estimate in (None, "first", "last")
        # a name is a word of a FASTA header line and of an @SQ line, unlike every other (the device takes any bytes)
        assert len(set(t.names)) == len(t.names) == len(t.seqs) and all(1 <= len(x) <= 254 and x.isalnum() for x in (y.replace("_", "a") for y in t.names))
        assert t.xa_moved is None or (t.long_names and t.xa is not None)
        if t.paired:  # the reads an orientation turns keep to orient_model.revcomp's letters
            f1, f2 = om.FLIPS[t.orientation]
            assert all(set(r) <= set(b"ACGTN") for r in (t.reads[:t.n] if f1 else []) + (t.reads[t.n:] if f2 else []))


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
    return out | newer_features(t, w, out)


def _fields(text):
    return [l.split(b"\t") for l in text.splitlines()]


def newer_features(t, w, older):
    """... and of the places of the orientation, the mate tags, --sam-seq and --xa."""
    out = set()
    o = om.NAMES[t.orientation].upper()
    if t.paired and t.orientation != om.FR:
        out |= {"%s: %s" % (o, x) for x in older if x.startswith("a kept kind-")}
        out |= {"not FR: " + x for x in older if x in ("a chosen record that is not its mate's first", "a placed unmapped mate")}
        if older & {"ins == X", "ins == I > 0"}:
            out.add("not FR: an insert on a bound")
    if not t.paired and t.orientation != om.FR and t.mate_tags:
        out.add("single-end with an orientation and mate tags set")
    if t.quals_on_host and t.sam_seq:
        out.add("refused: qualities on the host and --sam-seq")
    if t.quals_on_host and t.paired and t.mate_tags:
        out.add("refused: qualities on the host and paired mate tags")
    # --sam-seq
    if t.sam_seq:
        turned = [l.split(b"\t") for l in ss.turned(w.mated)]
        if any(set(f[9]) - set(b"ACGTN") for f in turned):
            out.add("a turned line with a letter outside A C G T N")
        if t.paired:
            at = {(t.rnames[r].encode(), bool(r >= t.n), t.names[k["record"][1]].encode(), b"%d" % (k["record"][2] + 1)) for r, k in w.kept.items()}
            if any((f[0], bool(int(f[1]) & 0x80), f[2], f[3]) in at for f in turned):
                out.add("a turned line of a rescued mate")
        if any(xm.xa_of(l) is not None and xm.flag_of(l) & 16 and l.split(b"\t")[9] != b"*" for l in w.text.splitlines()):
            out.add("a turned line with XA folded onto it")
    # --xa
    if t.xa is not None:
        for slot in xm.slots(w.seq):
            c1, f = len(slot) - 1, xm.folded(slot, t.xa)
            out |= {"f = 1"} if f == 1 else {"f in 31-33"} if 31 <= f <= 33 else {"f >= 64"} if f >= 64 else set()
            if f < min(c1, t.xa):
                out.add("f stopped by the byte budget")
            if f == t.xa < c1:
                out.add("f = N < c - 1")
            total = 0
            for k, l in enumerate(slot[1:1 + min(c1, t.xa)]):  # the sums the budget test sees: those of the entries within N
                total += len(xm.entry(l))
                if total in (xm.MAX_BYTES, xm.MAX_BYTES + 1):
                    out.add("a prefix sum of B" if total == xm.MAX_BYTES else "a prefix sum of B + 1")
                if total > xm.MAX_BYTES:
                    break
        if any(e[3] == b"*" for l in w.text.splitlines() for e in xm.entries(l)):
            out.add("an XA entry with CIGAR *")
    # the mate tags
    if t.paired and t.mate_tags:
        for pair in mt.pairs(w.tagged):
            for m in (0, 1):
                own, other = pair[m], pair[m ^ 1]
                if own is None or other is None:
                    continue
                g = other[0].split(b"\t")
                if not int(g[1]) & 4 and g[5] == b"*":
                    out.add("mate tags: the other mate's CIGAR is *")
                if int(g[1]) & 4 and g[2] != b"*":
                    out.add("mate tags: the other mate is unmapped and placed")
        if any(kind == 1 for kind, _ in w.kinds.values()):
            out.add("mate tags: the other mate's primary line is a rescued record")
        if t.mapq and any(x.startswith(b"MQ:i:") and x != b"MQ:i:255" for f in _fields(w.mated) for x in f[11:]):
            out.add("mate tags with MAPQ: an MQ other than 255")
    return out


COVERAGE = ["a pair with more than 32 combinations", "a mate with more than 32 lines", "a kept kind-2 rescue", "a kept kind-1 rescue",
            "a kind-2 rescue with equal sums in both directions", "a rescue traced but not kept", "ins == X", "ins == I > 0",
            "a chosen record that is not its mate's first", "a mate whose lines are not in NM order", "a placed unmapped mate",
            "a pair with both mates unmapped", "a 0x8000 record among a filtered slot's lines", "a slot cut by max_hits and by strata",
            # the orientation
            "RF: a kept kind-1 rescue", "RF: a kept kind-2 rescue", "FF: a kept kind-1 rescue", "FF: a kept kind-2 rescue",
            "not FR: a chosen record that is not its mate's first", "not FR: a placed unmapped mate", "not FR: an insert on a bound",
            "single-end with an orientation and mate tags set",
            # --sam-seq
            "a turned line with a letter outside A C G T N", "a turned line of a rescued mate", "a turned line with XA folded onto it",
            # --xa
            "f = 1", "f in 31-33", "f >= 64", "f stopped by the byte budget", "f = N < c - 1", "an XA entry with CIGAR *",
            "a prefix sum of B", "a prefix sum of B + 1",
            # the mate tags
            "mate tags: the other mate's CIGAR is *", "mate tags: the other mate is unmapped and placed",
            "mate tags: the other mate's primary line is a rescued record", "mate tags with MAPQ: an MQ other than 255",
            # the refusal
            "refused: qualities on the host and --sam-seq", "refused: qualities on the host and paired mate tags"]


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
    kept = {k: t.__dict__.pop(k) for k in ("_rescued", "_plain") if k in t.__dict__}  # (nothing made while patched is kept)
    pm.np = _LastOfTheLeast()
    try:
        return fl.expected(t, full=False).text
    finally:
        pm.np = np
        t.__dict__.pop("_rescued", None), t.__dict__.pop("_plain", None)
        t.__dict__.update(kept)


def _true(t):
    return next(w for u, w in trials() if u is t)


def _behind(t, plain=None, **kw):
    """The stages behind `plain` (by default the trial's own) alone: what a perturbation of a later stage recomputes."""
    w = types.SimpleNamespace(plain=_true(t).plain if plain is None else plain)
    return fl.lines_behind(t, w, **kw).text


def _other_orientation(t):
    return om.RF if t.orientation == om.FF else om.FR


def _other_orientation_defined(t):
    """... where the reads that go through a rescue model under it keep to orient_model.revcomp's letters."""
    if not t.paired or t.orientation == om.FR:
        return False
    f1, f2 = om.FLIPS[_other_orientation(t)]
    turned = (t.reads[:t.n] if f1 else []) + (t.reads[t.n:] if f2 else [])
    return not t.rescue or all(set(r) <= set(b"ACGTN") for r in turned)


def _replaced(text, line):
    """`text` with line(fields) -> fields on every line."""
    return b"".join(b"\t".join(line(l.split(b"\t"))) + b"\n" for l in text.splitlines())


def _tlen_by_real_strand(t):
    def line(f):
        if int(f[1]) & 2 and f[8] != b"0":
            f[8] = b"%d" % (-abs(int(f[8])) if int(f[1]) & 16 else abs(int(f[8])))
        return f
    return _behind(t, _replaced(_true(t).plain, line))


def _mate_strand_virtual(t):
    def line(f):
        flag = int(f[1])
        if om.FLIPS[t.orientation][0 if flag & 0x80 else 1] and not flag & 8:
            f[1] = b"%d" % (flag ^ 0x20)
        return f
    return _behind(t, _replaced(_true(t).plain, line))


def _patched(module, name, value, text):
    """text(t) with module.name = value(t)."""
    def run(t):
        old = getattr(module, name)
        setattr(module, name, value(t))
        try:
            return text(t)
        finally:
            setattr(module, name, old)
    return run


def _entry_by_virtual_strand(t):
    entry = xm.entry

    def virtual(line):
        flag = xm.flag_of(line)
        if om.FLIPS[t.orientation][1 if flag & 0x80 else 0]:
            f = line.split(b"\t")
            f[1] = b"%d" % (flag ^ 16)
            line = b"\t".join(f)
        return entry(line)
    return virtual


def _xa_before_filter(t):
    """The filter sparing a slot's first N secondary lines, which then fold: folding in front of the filter."""
    out = []
    for slot in rp.slots(fl.expected(t, full=False, strata=None, max_hits=None).plain):
        if int(slot[0].split(b"\t", 2)[1]) & 4:
            out += slot
            continue
        keep = rp.keep([rp.line_nm(l) for l in slot], t.strata, t.max_hits)
        out += [l for i, (l, k) in enumerate(zip(slot, keep)) if k or 1 <= i <= t.xa]
    return _behind(t, b"".join(out))


def _mates_from_single_end(t):
    """MC and MQ from the CIGAR and MAPQ columns of the other mate's first single-end record, not of its primary line: the tags
    mate_tags_model gives a text whose primary lines carry those columns, put onto the true lines."""
    e = t.e if t.mapq else None
    first = [s[0].split(b"\t") for s in rp.slots(rp.single_end(t.se, t.names, t.reads, t.rnames, t.quals, e=e, unmapped=True)[0])]
    assert len(first) == 2 * t.n
    reads = {}
    for r, name in enumerate(t.rnames):
        reads.setdefault((name.encode(), r >= t.n), []).append(r)

    def line(f):
        flag, at = int(f[1]), reads[(f[0], bool(int(f[1]) & 0x80))]
        if not flag & 0x104 and len(at) == 1 and not int(first[at[0]][1]) & 4:
            f[4], f[5] = first[at[0]][4], first[at[0]][5]
        return f
    true = _true(t).tagged
    doctored = _replaced(true, line)
    tagged = mt.apply(doctored, t.n, t.quals)
    mated = b"".join(a + o[len(d):] + b"\n" for a, d, o in zip(true.splitlines(), doctored.splitlines(), tagged.splitlines()))
    seq = ss.apply(mated) if t.sam_seq else mated
    return seq if t.xa is None else xm.apply(seq, t.xa)[0]


def _turn(seq_of, qual_of):
    def text(t):
        def line(f):
            if int(f[1]) & 16 and f[9] != b"*":
                f[9] = seq_of(f[9])
                f[10] = f[10] if f[10] == b"*" else qual_of(f[10])
            return f
        seq = _replaced(_true(t).mated, line)
        return seq if t.xa is None else xm.apply(seq, t.xa)[0]
    return text


_ACGT_ALONE = bytes(b"TGCA"[b"ACGT".index(c)] if c in b"ACGT" else ord("N") for c in range(256))

# the parameter a device might have one off, or the strand it might read: where it is defined for a trial, the expected text with it
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
    "another orientation": (_other_orientation_defined, lambda t: fl.expected(t, full=False, orientation=_other_orientation(t)).text),
    "TLEN's sign from the real strand": (lambda t: t.paired and t.orientation != om.FR, _tlen_by_real_strand),
    "0x20 from the virtual strand": (lambda t: t.paired and t.orientation != om.FR, _mate_strand_virtual),
    "XA N - 1": (lambda t: t.xa is not None and t.xa >= 2, lambda t: _behind(t, xa=t.xa - 1)),
    "XA N + 1": (lambda t: t.xa is not None and t.xa < xm.ALL, lambda t: _behind(t, xa=t.xa + 1)),
    "XA budget - 1": (lambda t: t.xa is not None, lambda t: _behind(t, xa_bytes=xm.MAX_BYTES - 1)),
    "XA budget + 1": (lambda t: t.xa is not None, lambda t: _behind(t, xa_bytes=xm.MAX_BYTES + 1)),
    "XA sign from the virtual strand": (lambda t: t.xa is not None and t.paired and t.orientation != om.FR,
                                        _patched(xm, "entry", _entry_by_virtual_strand, _behind)),
    "XA folded before the filter": (lambda t: t.xa is not None and (t.strata is not None or t.max_hits is not None), _xa_before_filter),
    "ms threshold 14": (lambda t: t.paired and t.mate_tags, _patched(mt, "MIN_QUAL", lambda t: 14, _behind)),
    "ms threshold 16": (lambda t: t.paired and t.mate_tags, _patched(mt, "MIN_QUAL", lambda t: 16, _behind)),
    "MC and MQ from the other mate's first single-end record": (lambda t: t.paired and t.mate_tags, _mates_from_single_end),
    "QUAL not reversed": (lambda t: t.sam_seq, _turn(ss.revcomp, lambda q: q)),
    "SEQ complemented by the A C G T table alone": (lambda t: t.sam_seq, _turn(lambda s: s.translate(_ACGT_ALONE)[::-1], lambda q: q[::-1])),
}
# ("secondary lines turned too" is not here: a secondary line prints * for SEQ and QUAL, and the model cannot turn a *.)


@pytest.mark.parametrize("what", sorted(PERTURBATIONS))
def test_sensitivity(what):
    defined, text = PERTURBATIONS[what]
    seen = sum(1 for t, w in trials() if defined(t) and text(t) != w.text)
    assert seen >= MIN_SENSITIVE, "%s changes the expected text of %d trials" % (what, seen)
    assert rm.ANCHORS == 8
