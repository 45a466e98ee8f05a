"""The model side of tests/fuzz_lines.py, without a GPU, on the exact (seed, trial) list of tests/test_gpu_fuzz_lines.py: draw()
is a function of (seed, trial) alone; the slice reaches the places where the kernels of fem_tail.hip go wrong (wave paths, ties,
inserts on a bound, lines out of NM order, the filter on 0x8000 records, rescues of either kind under RF and FF, turned lines with
IUPAC letters, folds of 1, 31-33 and 64 or more entries, the byte budget met exactly, the mate tags of rescued, placed and
untraced mates, the refusal of host qualities, kept parts at the floor and below 37 + 12e, clips on reverse lines and in MC:Z,
an XA byte budget met by the clip bytes, a3 against v3, one-base overlap cuts, tandem repeats, pairs proper only once cut, the
refusals of a trimmed batch's staging, fixed trims larger than a read, coverage windows larger than a sequence and spans
across two, ...); and an off-by-one in any parameter of the rule, or a strand taken from the wrong one of the real and the
virtual world, changes the expected text (or the expected track) of some trial, so that a device with it could not pass.
The figures are conditions on the committed slice: a seed list that misses one is changed, never the condition.

A perturbation recomputes only the stages behind the one it touches (fuzz_lines keeps a trial's records and its text up to
real_text per parameter set; lines_behind makes the rest).  The file took 14 s before the orientation, the mate tags, --sam-seq
and --xa were drawn (48 trials, 24 conditions) and took 30 s with them (72 trials, 63 conditions), on the same machine; 28 s
before the cut stage and the coverage track were drawn and 61 s with them (120 trials, 115 conditions), on one machine again:
a perturbation of the cut stage has the oracle map the batch's other kept parts and runs every stage, so test_cut_sensitivity
stops at the trials it needs."""
import functools
import types

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import adapter_model as adm
from tests import cases
from tests import coverage_model as cvm
from tests import fuzz_lines as fl
from tests import mate_tags_model as mt
from tests import orient_model as om
from tests import overlap_model as ovm
from tests import pair_model as pm
from tests import report_model as rp
from tests import rescue_model as rm
from tests import sam_seq_model as ss
from tests import trim_model as trm
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
    older = [t for c in fl.SLICE[:6] for t in by_id[c[0]]]
    assert len(older) == 72 and not any(t.trim or t.adapter or t.overlap or t.coverage or t.made for t in older)
    assert all(t.adapter and (t.overlap or not t.paired) for k in ("cuts", "cuts-pairs", "cuts-command-line") for t in by_id[k])
    assert all(t.trim for k in ("cuts", "cuts-pairs") for t in by_id[k])
    assert all(t.paired and t.overlap for t in by_id["cuts-pairs"]) and all(t.coverage for t in by_id["coverage"])
    assert sum(t.cli and t.paired for t in by_id["cuts-command-line"]) == 1
    # the new cases' command-line trial: the quality rule and a 3' trim, the track with a MAPQ bound that leaves lines on either
    # side, summed over several batches (FEM map --trim3 / --trim-qual / --coverage* and the BED file run in the slice)
    (_, seed, _, _, (k,)), t = fl.SLICE[-1], next(t for t in by_id["cuts-command-line"] if t.cli)
    fl.draw_cli(t, seed, k)
    assert t.trim and t.trim[1] > 0 and t.trim[2] > 0 and t.adapter and t.overlap and t.mapq and t.coverage and 0 < t.coverage[2] and t.batch < t.n
    mapqs = [int(f[4]) for f in _fields(fl.expected(t, full=False).text) if not int(f[1]) & 0x104 and f[5] != b"*"]
    assert min(mapqs) < t.coverage[2] <= max(mapqs) and any(t.coverage[0] < len(s) for s in t.seqs)
    for t, _ in trials():  # the drawn ranges
        assert 37 + 12 * t.e <= min(t.L, t.L2) and max(t.L, t.L2) <= 260 and 0 <= t.E <= 15 and 0 <= t.I <= t.X
        assert not t.rescue or t.X - t.I <= 65536
        assert all(1 <= len(x) <= 254 for x in t.rnames) and (t.rg is None or 1 <= len(t.rg) <= 255)
        assert not t.packed or (t.L == t.L2 and all(len(r) == t.L for r in t.reads))
        assert t.orientation in (0, 1, 2) and (t.xa is None or 1 <= t.xa <= 2 ** 31 - 1) and t.estimate in (None, "first", "last")
        # a name is a word of a FASTA header line and of an @SQ line, unlike every other (the device takes any bytes)
        assert len(set(t.names)) == len(t.names) == len(t.seqs) and all(1 <= len(x) <= 254 and x.isalnum() for x in (y.replace("_", "a") for y in t.names))
        assert t.xa_moved is None or (t.long_names and t.xa is not None)
        # the newest options' ranges: fem_dev_set_trim, _adapter, _pair_overlap, _coverage
        assert t.trim is None or (all(0 <= x <= 1024 for x in t.trim[:2]) and 0 <= t.trim[2] <= 93 and any(t.trim))
        assert t.adapter is None or (1 <= t.adapter[2] <= min(len(x) for x in t.adapter[:2] if x) and 0 <= t.adapter[3] <= 30 and
                                     all(4 <= len(x) <= 64 and set(x) <= set(b"ACGT") for x in t.adapter[:2] if x))
        assert t.overlap is None or (t.paired and 8 <= t.overlap[0] <= 1024 and 0 <= t.overlap[1] <= 30)
        assert t.coverage is None or (1 <= t.coverage[0] <= 1000000 and 0 <= t.coverage[2] <= 60)
        assert not (t.trim or t.adapter or t.overlap) or (not t.packed and all(33 <= ord(ch) <= 126 for q in t.quals for ch in q))
        assert not t.cli or not t.coverage or t.mapq or t.coverage[2] == 0
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
    return out | newer_features(t, w, out) | cut_features(t, w) | track_features(t, w)


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


def _cut_on(t):
    return bool(t.trim or t.adapter or t.overlap)


def _ops(cigar):
    return [(int(n), o) for n, o in cvm._OPS.findall(cigar)]


def _fixed_parts(t):
    """What the fixed trims leave of every read."""
    t5, t3, _ = t.trim or (0, 0, 0)
    out = []
    for r in t.reads:
        c5 = min(t5, len(r))
        out.append(r[c5:len(r) - min(t3, len(r) - c5)])
    return out


def cut_features(t, w):
    """... of the places of the cut stage: trimming, the adapter, the mates' overlap."""
    out = set()
    if t.packed_first:
        out.add("refused: a packed batch with a cut on")
    if not _cut_on(t):
        return out
    v, n, lo = fl.cut_view(t), t.n, 37 + 12 * t.e
    Q = (t.trim or (0, 0, 0))[2]
    if t.trim and max(t.trim[:2]) > max(len(r) for r in t.reads):
        out.add("t5 or t3 larger than a read")
    if t.quals_on_host:
        out.add("refused: --trim-qual mapped with the qualities on the host" if Q > 0 else "refused: a trimmed batch's text with the qualities on the host")
    lines = _fields(w.seq)
    printed = set(w.line_reads)
    if any(len(t.reads[r]) and not len(v.reads[r]) and r in printed for r in range(2 * n)):
        out.add("a read whose kept part is empty and whose line prints the whole read")
    if any(0 < len(v.reads[r]) < lo <= len(t.reads[r]) for r in range(2 * n)):
        out.add("a kept part below 37 + 12e")
    if Q > 0:
        lower = _floor(34)(t)
        if any(len(v.reads[r]) == trm.MIN_KEEP and lower.clips[r][1] > v.clips[r][1] for r in range(2 * n)):
            out.add("a quality cut stopped by the 35-base floor")
    mapped = [(f, r) for f, r in zip(lines, w.line_reads) if not int(f[1]) & 4 and f[5] != b"*"]
    if any(int(f[1]) & 16 and v.clips[r][0] != v.clips[r][1] and min(v.clips[r]) > 0 for f, r in mapped):
        out.add("a reverse-strand line with c5 != c3, both > 0")
    if t.paired:
        if any(sum(v.clips[r]) for r in w.kept):
            out.add("a rescued mate with clips")
        primary_rev = {r: bool(int(f[1]) & 16) for f, r in mapped if not int(f[1]) & 0x100}
        for f, r in mapped:
            o = r - n if r >= n else r + n
            if any(x.startswith(b"MC:Z:") for x in f[11:]) and primary_rev.get(o) and v.clips[o][0] != v.clips[o][1] and v.clips[o] != v.clips[r] and \
                    primary_rev.get(o) != bool(int(f[1]) & 16):
                out.add("an MC:Z whose clips are the other mate's, on a reverse primary")
        if any(sum(v.clips[r]) for f, r in mapped) and t.orientation != om.FR:
            out.add("cuts under %s" % om.NAMES[t.orientation].upper())
        proper = {r % n for f, r in mapped if int(f[1]) & 2}
        if proper:
            whole = fl.expected(t, full=False, view=fl.cut_view(t, trim=None, adapter=None, overlap=None))
            if proper - {r % n for f, r in zip(_fields(whole.seq), whole.line_reads) if int(f[1]) & 2}:
                out.add("a pair that is proper only because of the cut")
    if v.a3 and v.v3:
        if any(a > x > 0 for a, x in zip(v.a3, v.v3)):
            out.add("a pair with a3 > v3 > 0")
        if any(x > a > 0 for a, x in zip(v.a3, v.v3)):
            out.add("a pair with v3 > a3 > 0")
    if v.v3:
        if 1 in v.v3:
            out.add("an overlap cut of exactly one base")
        parts, (O, E) = _fixed_parts(t), t.overlap
        for i in range(n):
            _, o, matches = ovm._profile(bytes(parts[i]), bytes(parts[n + i]))
            if int(((o >= O) & ((o - matches) * 100 <= o * E)).sum()) >= 2:
                out.add("a pair in which several f match")
                break
    if t.xa is not None:  # the byte budget's test sees the clipped entries: a sum that meets it with the clip bytes alone
        for clipped, bare in zip(xm.slots(w.seq), xm.slots(w.mated)):
            a = b = 0
            for lc, lb in zip(clipped[1:1 + t.xa], bare[1:1 + t.xa]):
                a, b = a + len(xm.entry(lc)), b + len(xm.entry(lb))
                if a in (xm.MAX_BYTES, xm.MAX_BYTES + 1) and b != a:
                    out.add("an XA prefix sum of B or B + 1 with the clip bytes and not without them")
                if a > xm.MAX_BYTES:
                    break
    return out


def _counts_in_track(t, f):
    """Rule 1 of the track on the columns of one line."""
    _, all_hits, min_mapq = t.coverage
    return not int(f[1]) & 4 and (all_hits or not int(f[1]) & 0x100) and f[5] != b"*" and int(f[4]) >= min_mapq


def track_features(t, w):
    """... and of the places of the coverage track."""
    out = set()
    if not t.coverage:
        return out
    W, all_hits, min_mapq = t.coverage
    lens = dict(zip((x.encode() for x in t.names), (len(s) for s in t.seqs)))
    if W > min(lens.values()):
        out.add("W larger than a sequence")
    for f in _fields(w.seq):  # (the lines in front of the folding: a folded line counts as the line it was)
        if f[5] == b"*" or int(f[1]) & 4:
            continue
        if min_mapq > 0 and int(f[4]) == min_mapq and (all_hits or not int(f[1]) & 0x100):
            out.add("a line whose MAPQ equals min_mapq")
        if not _counts_in_track(t, f):
            continue
        pos0, s, n = int(f[3]) - 1, cvm.span(f[5]), lens[f[2]]
        end = min(pos0 + s, n)
        if pos0 // W != (end - 1) // W:
            out.add("a counting line that spans two windows")
        if n % W and n > W and (end - 1) // W == n // W:
            out.add("a span in a sequence's last, shorter window")
        if any(o == b"D" for _, o in _ops(f[5])):
            out.add("a counting line with a D operation")
    if all_hits and t.xa is not None and not np.array_equal(_without_xa_entries(t), w.bins):
        out.add("a counted XA entry under all_hits")
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
            "refused: qualities on the host and --sam-seq", "refused: qualities on the host and paired mate tags",
            # the cut stage
            "a read whose kept part is empty and whose line prints the whole read", "a kept part below 37 + 12e",
            "a quality cut stopped by the 35-base floor", "a reverse-strand line with c5 != c3, both > 0", "a rescued mate with clips",
            "an MC:Z whose clips are the other mate's, on a reverse primary",
            "an XA prefix sum of B or B + 1 with the clip bytes and not without them", "a pair with a3 > v3 > 0", "a pair with v3 > a3 > 0",
            "an overlap cut of exactly one base", "a pair in which several f match", "a pair that is proper only because of the cut",
            "cuts under RF", "cuts under FF", "t5 or t3 larger than a read", "refused: a packed batch with a cut on",
            "refused: --trim-qual mapped with the qualities on the host", "refused: a trimmed batch's text with the qualities on the host",
            # the coverage track
            "a counting line that spans two windows", "a span in a sequence's last, shorter window", "a counting line with a D operation",
            "a counted XA entry under all_hits", "a line whose MAPQ equals min_mapq", "W larger than a sequence"]


@functools.lru_cache(maxsize=None)
def found():
    return [features(t, w) for t, w in trials()]


@pytest.mark.parametrize("what", COVERAGE)
def test_coverage(what):
    hits = sum(what in f for f in found())
    assert hits >= MIN_TRIALS, "%s: in %d of %d trials" % (what, hits, len(found()))


def test_most_trials_map_something():
    assert 10 * sum("nothing maps" in f for f in found()) <= len(found())


@pytest.mark.parametrize("case", [c[0] for c in fl.SLICE if c[0].startswith("cuts")])
def test_the_cuts_make_their_reads_mappable(case):
    """The as-if property is compared on reads that map: of the reads that cases.cut_pairs made with a tail, an adapter or a
    read-through, at least half have a record on their kept part, and none of those with 8 foreign bases or more has one on
    the read as given (the oracle alone, at the trial's e; cases.cut_pairs makes such a tail of cases.long_tail(e) bases at the
    least, which is asserted here too)."""
    seed = next(c[1] for c in fl.SLICE if c[0] == case)
    made = kept = 0
    for (t, _), (s, _, _) in zip(trials(), fl.slice_trials()):
        if s != seed:
            continue
        cnt = np.diff(t.se.rec_off.astype(np.int64))
        made, kept = made + len(t.made), kept + sum(int(cnt[r] > 0) for r, _ in t.made)
        long = [r for r, tail in t.made if tail >= 8]
        assert all(tail < 8 or tail >= cases.long_tail(t.e) for _, tail in t.made)
        whole = fo.map_reads(t.ref, t.idx, fo.ReadBatch([t.reads[r] for r in long]), e=t.e, threads=fl.THREADS)
        assert int(whole.rec_off[-1]) == 0, "%s: reads map as they are given" % case
    assert made >= 100 and 2 * kept >= made, "%s: %d of %d made reads map once cut" % (case, kept, made)


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


def _behind(t, plain=None, line_reads=None, **kw):
    """The stages behind `plain` (by default the trial's own) alone: what a perturbation of a later stage recomputes."""
    w = types.SimpleNamespace(plain=_true(t).plain if plain is None else plain, line_reads=_true(t).line_reads if line_reads is None else line_reads)
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
    out, reads = [], []
    whole = fl.expected(t, full=False, strata=None, max_hits=None)
    of_line = iter(whole.line_reads)
    for slot in rp.slots(whole.plain):
        keep = [True] * len(slot) if int(slot[0].split(b"\t", 2)[1]) & 4 else rp.keep([rp.line_nm(l) for l in slot], t.strata, t.max_hits)
        for i, (l, k) in enumerate(zip(slot, keep)):
            r = next(of_line)
            if k or 1 <= i <= t.xa:
                out.append(l)
                reads.append(r)
    return _behind(t, b"".join(out), reads)


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
    # (these three rebuild stages of a text without soft clips; with a cut on the clip stage makes SEQ, QUAL and the mate tags'
    # clips, and CUT_PERTURBATIONS below holds that stage's order and strands)
    "MC and MQ from the other mate's first single-end record": (lambda t: t.paired and t.mate_tags and not _cut_on(t), _mates_from_single_end),
    "QUAL not reversed": (lambda t: t.sam_seq and not _cut_on(t), _turn(ss.revcomp, lambda q: q)),
    "SEQ complemented by the A C G T table alone": (lambda t: t.sam_seq and not _cut_on(t),
                                                    _turn(lambda s: s.translate(_ACGT_ALONE)[::-1], lambda q: q[::-1])),
}
# ("secondary lines turned too" is not here: a secondary line prints * for SEQ and QUAL, and the model cannot turn a *.)


@pytest.mark.parametrize("what", sorted(PERTURBATIONS))
def test_sensitivity(what):
    defined, text = PERTURBATIONS[what]
    seen = sum(1 for t, w in trials() if defined(t) and text(t) != w.text)
    assert seen >= MIN_SENSITIVE, "%s changes the expected text of %d trials" % (what, seen)
    assert rm.ANCHORS == 8


# ---- the cut stage: a parameter one off, or a step of the rule taken another way ----

def _cut_text(t, **kw):
    """The expected text with the cut stage's settings replaced (cut_view's arguments): the oracle maps the other kept parts."""
    return fl.expected(t, full=False, view=fl.cut_view(t, **kw)).text


def _variant(tag, module, name, value):
    """-> view(t): the cut view with module.name = value while the clips are made."""
    def view(t):
        old = getattr(module, name)
        setattr(module, name, value)
        try:
            return fl.cut_view(t, tag=tag)
        finally:
            setattr(module, name, old)
    return view


def _floor(k):
    return _variant("the floor at %d" % k, trm, "MIN_KEEP", k)


def _clips_at_equal_sums(qual_bytes, t5, t3, Q):
    """trim_model.clips with `s >= best`: among equal sums the least l, the largest cut."""
    b = bytes(qual_bytes)
    L = len(b)
    c5 = min(t5, L)
    c3f = min(t3, L - c5)
    Lp = L - c5 - c3f
    cut = Lp
    if Q >= 1 and Lp > trm.MIN_KEEP:
        s = best = 0
        for l in range(Lp - 1, trm.MIN_KEEP - 1, -1):
            s += Q - (b[c5 + l] - 33)
            if s < 0:
                break
            if s >= best:
                best, cut = s, l
    return c5, c3f + (Lp - cut)


def _last_p(x, A, O=adm.O, E=adm.E):
    """adapter_model.cut with the last matching p in place of the least."""
    x, A = adm._bytes(x), adm._bytes(A).upper()
    hits = [p for p in range(len(x)) if min(len(A), len(x) - p) >= O and
            sum(1 for j in range(min(len(A), len(x) - p)) if adm._upper(x[p + j]) != A[j]) * 100 <= min(len(A), len(x) - p) * E]
    return len(x) - hits[-1] if hits else 0


def _least_f(x, y, O=ovm.O, E=ovm.E):
    f, o, matches = ovm._profile(ovm._bytes(x), ovm._bytes(y))
    hit = (o >= O) & ((o - matches) * 100 <= o * E)
    return int(f[hit].min()) if hit.any() else 0


def _composed(how):
    """-> view(t): the producers' cuts put together another way: "sum": a3 + v3 in place of the larger one; "quality first": the
    quality rule on all the fixed trims leave, and the larger of its cut and the producers'."""
    def view(t):
        t5, t3, Q = t.trim or (0, 0, 0)
        true = fl.cut_view(t)
        cl = []
        for r, q, a, x in zip(t.reads, t.quals, true.a3 or [0] * len(t.reads), true.v3 or [0] * len(t.reads)):
            L, qb = len(r), q.encode("latin-1")
            c5 = min(t5, L)
            c3f = min(t3, L - c5)
            if how == "sum":
                cut = min(a + x, L - c5 - c3f)
                cut += trm.clips(qb[c5:L - c3f - cut], 0, 0, Q)[1]
            else:
                cut = max(a, x, trm.clips(qb[c5:L - c3f], 0, 0, Q)[1])
            cl.append((c5, c3f + cut))
        return fl.cut_view(t, tag=how, clips=(cl, true.a3, true.v3))
    return view


def _of_view(view):
    return lambda t: fl.expected(t, full=False, view=view(t)).text


def _unswapped(cigar, c5, c3, reverse):
    return _clip_cigar(cigar, c5, c3, False)


_clip_cigar = trm.clip_cigar


def _tag_from(t, prefix, value):
    """The expected text with `prefix` tags replaced: value(the line's fields in front of the clip stage, its read, the tag) -> the
    tag's bytes; XA folded behind it as ever."""
    w = _true(t)
    out = []
    for bare, f, r in zip(_fields(w.mated), _fields(w.seq), w.line_reads):
        out.append(b"\t".join(value(bare, r, x) if x.startswith(prefix) else x for x in f) + b"\n")
    seq = b"".join(out)
    return seq if t.xa is None else xm.apply(seq, t.xa)[0]


def _mc_by_own_strand(t):
    v, n = fl.cut_view(t), t.n

    def value(bare, r, x):
        o = r - n if r >= n else r + n
        kept = next(y for y in bare[11:] if y.startswith(b"MC:Z:"))[5:]
        return b"MC:Z:" + _clip_cigar(kept, v.clips[o][0], v.clips[o][1], bool(int(bare[1]) & 16))
    return _tag_from(t, b"MC:Z:", value)


def _ms_over_kept(t):
    return _tag_from(t, b"ms:i:", lambda bare, r, x: next(y for y in bare[11:] if y.startswith(b"ms:i:")))


def _xa_before_clips(t):
    """XA folded on the kept parts' text, the clip stage behind it: the budget then counts no clip bytes.  The text is folded
    under the reads' numbers for names (the folding reads no name), so that the clip stage finds each line's read."""
    w, v = _true(t), fl.cut_view(t)
    numbered = b"".join(b"%d\t" % (r % t.n if t.paired else r) + l.split(b"\t", 1)[1] + b"\n" for l, r in zip(w.mated.splitlines(), w.line_reads))
    folded = xm.apply(numbered, t.xa)[0]
    ids = ["%d" % r for r in range(t.n if t.paired else 2 * t.n)]
    text = trm.apply(folded, t.reads, t.quals, v.clips, ids, paired=t.paired, sam_seq=t.sam_seq)
    names = t.rnames
    return b"".join(names[int(l.split(b"\t", 1)[0])].encode("latin-1") + b"\t" + l.split(b"\t", 1)[1] + b"\n" for l in text.splitlines())


def _trim(i, d):
    return _setting("trim", i, d)


def _setting(key, i, d):
    return lambda t: _cut_text(t, **{key: tuple(x + d if k == i else x for k, x in enumerate(getattr(t, key)))})


_Q = lambda t: (t.trim or (0, 0, 0))[2]  # noqa: E731

CUT_PERTURBATIONS = {
    "t5 + 1": (lambda t: t.trim and t.trim[0] < 1024, _trim(0, 1)),
    "t3 + 1": (lambda t: t.trim and t.trim[1] < 1024, _trim(1, 1)),
    "Q - 1": (lambda t: _Q(t) >= 1, _trim(2, -1)),
    "Q + 1": (lambda t: 1 <= _Q(t) <= 92, _trim(2, 1)),
    "the floor at 34": (lambda t: _Q(t) >= 1, _of_view(_floor(34))),
    "the floor at 36": (lambda t: _Q(t) >= 1, _of_view(_floor(36))),
    "s >= best in place of s > best": (lambda t: _Q(t) >= 1, _of_view(_variant("s >= best", trm, "clips", _clips_at_equal_sums))),
    "adapter O + 1": (lambda t: t.adapter and t.adapter[2] < min(len(t.adapter[0]), len(t.adapter[1] or t.adapter[0])), _setting("adapter", 2, 1)),
    "adapter E - 1": (lambda t: t.adapter and t.adapter[3] >= 1, _setting("adapter", 3, -1)),
    "the second mates matched against A": (lambda t: t.adapter and t.adapter[1] and t.paired,
                                           lambda t: _cut_text(t, adapter=(t.adapter[0], None) + t.adapter[2:])),
    "the last matching p in place of the least": (lambda t: t.adapter, _of_view(_variant("the last p", adm, "cut_np", _last_p))),
    "overlap O + 1": (lambda t: t.overlap and t.overlap[0] < 1024, _setting("overlap", 0, 1)),
    "overlap E - 1": (lambda t: t.overlap and t.overlap[1] >= 1, _setting("overlap", 1, -1)),
    "the least matching f in place of the largest": (lambda t: t.overlap, _of_view(_variant("the least f", ovm, "frag_np", _least_f))),
    "a3 + v3 in place of the larger": (lambda t: t.adapter and t.overlap, _of_view(_composed("sum"))),
    "the quality rule in front of the adapter's cut": (lambda t: _Q(t) >= 1 and (t.adapter or t.overlap), _of_view(_composed("quality first"))),
    "the clips not swapped on 0x10 lines": (_cut_on, _patched(trm, "clip_cigar", lambda t: _unswapped, _behind)),
    "MC's clips swapped by the line's own strand": (lambda t: _cut_on(t) and t.paired and t.mate_tags, _mc_by_own_strand),
    "ms over the kept qualities": (lambda t: _cut_on(t) and t.paired and t.mate_tags, _ms_over_kept),
    "XA folded in front of the clip stage": (lambda t: _cut_on(t) and t.xa is not None, _xa_before_clips),
}


@pytest.mark.parametrize("what", sorted(CUT_PERTURBATIONS))
def test_cut_sensitivity(what):
    """As test_sensitivity; the trials are walked until MIN_SENSITIVE of them have shown the perturbation (each of these maps
    the batch's other kept parts with the oracle and runs every stage again)."""
    defined, text = CUT_PERTURBATIONS[what]
    seen = 0
    for t, w in trials():
        if defined(t) and text(t) != w.text:
            seen += 1
            if seen >= MIN_SENSITIVE:
                break
    assert seen >= MIN_SENSITIVE, "%s changes the expected text of %d trials" % (what, seen)


# ---- the coverage track: the bins, not the text ----

def _span_with(counted):
    def span(cigar):
        if cigar == b"*":
            return None
        return sum(n for n, o in _ops(cigar) if o in counted)
    return span


def _track_with(name, value, **kw):
    def bins(t):
        old = getattr(cvm, name)
        setattr(cvm, name, value)
        try:
            return fl.track(t, _true(t), **kw)
        finally:
            setattr(cvm, name, old)
    return bins


_lines = cvm.lines


def _without_xa_entries(t):
    """The track of the expected text as it stands, its XA entries passed over (at every min_mapq: a line that stayed a line
    carries its MAPQ)."""
    W, all_hits, q = t.coverage
    cvm.lines = lambda text: [x[:5] + ([],) for x in _lines(text)]
    try:
        return cvm.bins(_true(t).text, t.names, [len(s) for s in t.seqs], W, all_hits, q)
    finally:
        cvm.lines = _lines


def _mapq_track(t, d):
    """(where XA folds under all_hits the track reads the text in front of the folding, as fuzz_lines.track does at min_mapq > 0)"""
    W, all_hits, q = t.coverage
    w = _true(t)
    return cvm.bins(w.seq if all_hits else w.text, t.names, [len(s) for s in t.seqs], W, all_hits, q + d)


TRACK_PERTURBATIONS = {
    "W - 1": (lambda t: t.coverage and t.coverage[0] >= 2, lambda t: fl.track(t, _true(t), window=t.coverage[0] - 1)),
    "W + 1": (lambda t: t.coverage, lambda t: fl.track(t, _true(t), window=t.coverage[0] + 1)),
    "soft clips counted as covered": (lambda t: t.coverage and _cut_on(t), _track_with("span", _span_with((b"M", b"D", b"S")))),
    "insertions counted": (lambda t: t.coverage, _track_with("span", _span_with((b"M", b"D", b"I")))),
    "min_mapq - 1": (lambda t: t.coverage and t.mapq and t.coverage[2] >= 1, lambda t: _mapq_track(t, -1)),
    "min_mapq + 1": (lambda t: t.coverage and t.mapq, lambda t: _mapq_track(t, 1)),
    "all_hits leaving out the XA entries": (lambda t: t.coverage and t.coverage[1] and t.xa is not None, _without_xa_entries),
    # (twice the bins differ from the bins of every track that is not empty: this one shows only that some line of the trial
    # counts.  That a second add would be seen is fuzz_lines.compare()'s doing, which reads the track behind all of its fetches.)
    "a second fetch counted again": (lambda t: t.coverage, lambda t: 2 * _true(t).bins),
}


@pytest.mark.parametrize("what", sorted(TRACK_PERTURBATIONS))
def test_track_sensitivity(what):
    defined, bins = TRACK_PERTURBATIONS[what]
    seen = sum(1 for t, w in trials() if defined(t) and bins(t).tobytes() != w.bins.tobytes())
    assert seen >= MIN_SENSITIVE, "%s changes the expected track of %d trials" % (what, seen)
