"""Randomised differential run of the output-line options: pairing, mate rescue, --rescue-discordant, MAPQ, the unmapped reads'
lines, --strata / --max-hits, the RG / NH / HI tags, the library's orientation (FR, RF, FF), --mate-tags, --sam-seq, --xa (its
entry limit and its byte budget, with long reference names), the two library estimates and BAM, all drawn together, against the
composed plain-Python models (tests/pair_model, rescue_model, discordant_model, mapq_model, unmapped_model, report_model,
orient_model, tags_model, mate_tags_model, sam_seq_model, xa_model, bam_model) on the oracle's single-end records.
include/fem_hip.h is the arbiter, and expected() composes the models in the order it states.

In front of them the cut stage is drawn: the fixed trims and the quality rule (fem_dev_set_trim), the 3' adapter with a second
one for the second mates (fem_dev_set_adapter) and the mates' overlap (fem_dev_set_pair_overlap), composed by overlap_model /
adapter_model / trim_model; and beside them the coverage track (fem_dev_set_coverage; coverage_model on the expected text, never
on the device's).  A trial with a cut on gets cases.cut_pairs' reads, which map only once they are cut: bad-quality tails,
adapter read-through, pairs read through their fragment, tandem repeats.  The as-if property is what is composed: the oracle
maps the kept parts, every older stage runs on them, trim_model.apply puts the soft clips, the whole SEQ and QUAL and ms:i in
(it turns SEQ and QUAL itself under --sam-seq), and XA folds last, its byte budget counting the clips.  The clip points and each
producer's cuts and counters are compared read for read, the refusals that the header states for a trimmed batch are expected
where the drawn staging meets them, and the track must hold the batch exactly once after every fetch compare() performs.

A paired trial's reads are an FR world's, turned with orient_model.virtual_reads before the oracle maps them, so the fixtures
and the moved insert bound mean under RF and FF what they mean under FR.  The mates an orientation turns hold upper-case
A C G T N only (the domain of orient_model.revcomp; the header defines no more): lower-case reads and the other IUPAC letters
go into every mate under FR, into mate 1 under FF, into none under RF, and into every read single-end, where nothing is turned
and the orientation, set all the same, must change nothing.  --infer-insert and --orientation auto stay with their own tests:
their sample is a file's head, not a trial's batch.

Every trial is three functions: draw(rng) makes the world and the options, expected(trial) runs the models (both on the CPU:
tests/test_fuzz_lines_model.py holds the drawn slice to coverage and sensitivity conditions), compare(dev, trial, want) runs the
device.  One Device serves the whole run, so what a trial leaves behind in a slot meets the next trial's options.

By the clock:  FUZZ_SECONDS=300 FUZZ_SEED=1 python tests/fuzz_lines.py ;  FUZZ_TRIAL=k re-runs trial k of the seed alone (a
trial's random stream is default_rng([seed, k])).  Not collected by pytest; a bounded slice with fixed seeds runs under
`pytest -m gpu` (tests/test_gpu_fuzz_lines.py)."""
import gzip
import itertools
import os
import pathlib
import struct
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from oracle import fem_oracle as fo
from tests import adapter_model as adm
from tests import bam_model as bm
from tests import coverage_model as cvm
from tests import discordant_fixture as df
from tests import insert_model as im
from tests import mate_tags_model as mt
from tests import orient_model as om
from tests import overlap_model as ovm
from tests import pair_model as pm
from tests import report_model as rp
from tests import rescue_model as rm
from tests import sam_seq_model as ss
from tests import tags_model as tm
from tests import trim_model as trm
from tests import unmapped_model as um
from tests import xa_model as xm
from tests import util
from tests.cases import CUT_PROFILES, cut_pairs, make_pairs, write_fastq
from tests.harness import build_index, decode_bam_file, first_difference, run_fem

THREADS = 8
COPIES = (6, 12, 40, 80)
IUPAC = b"NNNNRYKMSWBDHVn"
LETTERS = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", np.uint8)
INSERT_LISTS = 16  # the records of a mate that draw() looks at for inserts that occur
XA_LIMITS = (1, 2, 3, 31, 32, 33, 63, 64, 65, xm.ALL)  # a lane's slot and its last line, a wave's first, one step, two, no limit
LONG_NAME = (150, 241)  # the letters behind chr<i>_ of a long reference name: some forty entries fill FEM_XA_MAX_BYTES
OPTIONS = ("paired", "e", "E", "L", "L2", "I", "X", "rescue", "discordant", "mapq", "unmapped", "strata", "max_hits", "rg", "hits",
           "bam_level", "nowait", "packed", "quals_on_host", "slot", "copies", "n", "moved", "cli", "orientation", "mate_tags", "sam_seq",
           "xa", "estimate", "long_names", "xa_moved", "trim", "adapter", "overlap", "coverage", "packed_first", "records_first", "again")
# --trim-qual: off, the least ones, the usual ones, the largest (which cuts every read to the floor)
TRIM_QUALS = (0, 0, 1, 2, 2, 20, 20, 20, 20, 20, 30, 30, 93)
COVERAGE_WINDOWS = (1, 7, 64, 1000)  # ... and one more than the longest sequence, and a sequence's length


_KEEP = object()


def _printable(rng, n, lo=33):
    return bytes(rng.integers(lo, 127, size=n).astype(np.uint8))


def _qname(rng):
    """1..254 bytes of [!-~], a letter at either end (a FASTQ header line and a SAM header line begin with @; a mate suffix
    /1 /2 is cut off a name)."""
    n = int(rng.integers(1, 255)) if rng.random() < 0.3 else int(rng.integers(1, 40))
    s = bytearray(_printable(rng, n))
    s[0] = LETTERS[rng.integers(0, len(LETTERS))]
    s[-1] = LETTERS[rng.integers(0, len(LETTERS))]
    return bytes(s).decode("latin-1")


def occurring_inserts(se, n, I=0, X=1 << 30):
    """The inserts of the concordant record combinations of every pair under (I, X), by default (0, 2^30):
    pair_model.insert_of over each mate's first INSERT_LISTS records."""
    out = []
    for i in range(n):
        a0, a1 = int(se.rec_off[i]), int(se.rec_off[i + 1])
        b0, b1 = int(se.rec_off[n + i]), int(se.rec_off[n + i + 1])
        for ja in range(a0, min(a1, a0 + INSERT_LISTS)):
            for jb in range(b0, min(b1, b0 + INSERT_LISTS)):
                ins = pm.insert_of(se, ja, jb, I, X)
                if ins is not None:
                    out.append(ins)
    return out


def anchor_pairs(rng, L, L2, e, E, X, n_copies=9):
    """-> (a sequence, mate 1 reads, mate 2 reads): two pairs for the limit of rescue_model.ANCHORS.  Mate 1 of each is a segment
    that stands n_copies times in the sequence, exactly and too far apart to share a window, so its records tie; mate 2's segment,
    with e + 1 .. E substitutions (0 .. e where E <= e), stands beside one copy alone: the eighth for the first pair, any for the
    second, the ninth included, which no rescue reaches."""
    parts, r1, r2 = [util.rand_seq(rng, 500)], [], []
    for beside in (7, int(rng.integers(0, n_copies))):
        a, b = util.rand_seq(rng, L), util.rand_seq(rng, L2)
        k = int(rng.integers(e + 1, E + 1)) if E > e else int(rng.integers(0, e + 1))
        c = bytearray(b)
        for x in rng.choice(np.arange(2, L2 - 2), k, replace=False):
            c[int(x)] = ord("A") if c[int(x)] != ord("A") else ord("C")
        gap = int(rng.integers(20, X - max(L, L2) + 1))
        for j in range(n_copies):
            parts += [a, util.rand_seq(rng, gap)]
            parts += [bytes(c) if j == beside else util.rand_seq(rng, L2), util.rand_seq(rng, X + 300)]
        r1.append(a)
        r2.append(util.revcomp(b))
    return b"".join(parts), r1, r2


def draw(rng, force=None):
    """World and options of one trial: a random 60 kbp sequence, two or three repeat-rich ones, the discordant fixture's decoy and
    anchor_pairs' sequence; the fixture's pairs, anchor_pairs' and make_pairs', some mates made odd; the options, each drawn
    on its own; the oracle's records; the insert range, in most paired trials with a bound on an insert that occurs; the XA
    limit, from the ladder or from a slot that occurs, and with long reference names a name's length moved onto the byte budget
    (xa_moved); the cut stage and the coverage track (draw_cuts).  force: values that a caller fixes instead of drawing them (e,
    copies, cli, orientation, long_names, strata, max_hits, xa: the ladder's value; paired, or single_end: the share of
    single-end trials; mapq; trim, adapter, overlap, coverage: True draws the option on, False leaves it off)."""
    f = force or {}
    t = types.SimpleNamespace()
    o = rng.spawn(1)[0]  # the newer options draw from a child stream, so the older ones and the FR world stay what they were
    cr = rng.spawn(1)[0]  # ... and the cut stage and the coverage track from a further one
    t.orientation = int(f.get("orientation", o.integers(0, 3)))
    t.cli = bool(f.get("cli", False))
    e = int(rng.choice([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 6, 7]))  # (a forced value takes the place of a drawn one: the stream goes on alike)
    t.e = e = int(f.get("e", e))
    lo = 37 + 12 * e
    t.L = L = int(rng.integers(lo, 261))
    t.L2 = L2 = L if rng.random() < 0.5 else int(rng.integers(lo, 261))
    t.E = E = int(rng.integers(e + 1, 16)) if rng.random() < 0.75 else int(rng.integers(0, 16))
    X = int(rng.integers(max(L, L2) + 60, 901))
    t.copies = copies = int(f.get("copies", rng.choice(COPIES)))
    # the world
    main = [util.rand_seq(rng, 60_000)]
    main += util.repeat_rich_reference(rng, n_seq=int(rng.integers(2, 4)), unit_len=300, n_units=int(rng.choice([3, 4, 6])),
                                       copies=copies, spacer=200)
    nd = int(rng.integers(16, 41))
    seqs, r1, r2 = df.make_discordant_pairs(rng, main, nd, L, L2, e, E, X, n_sym=int(rng.integers(2, 7)),
                                            decoy_copies=int(rng.integers(1, 3)), near_end=bool(rng.integers(0, 2)))
    p1, p2 = make_pairs(rng, seqs, int(rng.integers(10, 41)), L, e, L2)
    tied, a1, a2 = anchor_pairs(rng, L, L2, e, E, X)
    seqs = seqs + [tied]
    for a, b in zip(a1, a2):  # (somewhere among the others, either mate first)
        at = int(rng.integers(0, len(r1) + 1))
        a, b = (a, b) if rng.integers(0, 2) else (b, a)
        r1.insert(at, a)
        r2.insert(at, b)
    r1, r2 = r1 + p1, r2 + p2
    t.n = n = len(r1)
    reads = r1 + r2
    # mode, staging
    t.paired = bool(f.get("paired", rng.random() >= f.get("single_end", 0.25)))
    t.packed = bool(L == L2 and rng.random() < 0.4)
    # odd reads: lower case (0x8000 records), N and IUPAC letters, random mates, reads of length 0.  The mates that a paired
    # trial's orientation flips keep to upper-case A C G T N (orient_model.revcomp's domain): the same draws, the letter left out
    flips = om.FLIPS[t.orientation] if t.paired else (0, 0)
    for r in rng.choice(2 * n, int(rng.integers(2, 5)), replace=False):
        if not flips[int(r >= n)]:
            reads[r] = reads[r].lower()
    for r in rng.choice(2 * n, int(rng.integers(2, 6)), replace=False):
        s = bytearray(reads[r])
        for x in rng.integers(0, len(s), int(rng.integers(1, 4))):
            c = IUPAC[int(rng.integers(0, len(IUPAC)))]
            s[int(x)] = c if not flips[int(r >= n)] else ord("N")
        reads[r] = bytes(s)
    for r in rng.choice(2 * n, int(rng.integers(1, 4)), replace=False):
        reads[r] = util.rand_seq(rng, len(reads[r]))
    if not t.packed and not t.cli:
        for r in rng.choice(2 * n, int(rng.integers(1, 3)), replace=False):
            reads[r] = b""
    if t.packed and 20 * sum(sum(c not in b"ACGT" for c in r) for r in reads) > 2 * n * L:
        t.packed = False  # (a batch with more than one odd byte in sixteen goes as characters)
    if t.paired:  # so far the FR world's reads; the library's are those turned (single-end nothing reads the orientation: no read is)
        reads = om.virtual_reads(reads, n, t.orientation)
    base = [_qname(rng) for _ in range(n)]
    quals = [_printable(rng, len(r)).decode("latin-1") for r in reads]
    seqs, reads, quals, base = draw_cuts(t, cr, f, seqs, reads, quals, base)
    t.n = n = len(base)
    t.seqs, t.reads, t.quals, t.rnames = seqs, reads, quals, base + base
    t.names = ["chr%d%s" % (i, "_x" * int(rng.integers(0, 20))) for i in range(len(seqs))]
    t.long_names = bool(f.get("long_names", o.random() < 0.3))
    if t.long_names:  # (as xa_model.long_names: the byte budget then stops a slot's folding at these repeat sizes)
        t.names = ["chr%d_%s" % (i, chr(97 + i % 26) * int(o.integers(*LONG_NAME))) for i in range(len(seqs))]
    # the output options
    t.rescue = bool(rng.random() >= 0.2)
    t.discordant = bool(rng.integers(0, 2))
    t.mapq = bool(f.get("mapq", rng.integers(0, 2)))
    t.unmapped = bool(rng.integers(0, 2))
    t.strata = None if rng.random() < 0.4 else int(rng.integers(0, 4)) if rng.random() < 0.75 else int(rng.integers(0, 16))
    u = rng.random()
    t.max_hits = None if u < 0.4 else (1 << 31) - 1 if u < 0.5 else int(rng.integers(1, 7))
    t.strata, t.max_hits = f.get("strata", t.strata), f.get("max_hits", t.max_hits)
    t.rg = None if rng.random() < 0.4 else _printable(rng, int(rng.integers(1, 256)) if rng.random() < 0.3 else int(rng.integers(1, 12)), 32)
    if t.cli and t.rg is not None:  # (FEM map --rg reads the two characters \t as a tab)
        t.rg = t.rg.replace(b"\\", b"/")
    t.hits = bool(rng.integers(0, 2))
    t.bam_level = int(rng.integers(0, 2))
    t.nowait = bool(rng.integers(0, 2))
    t.quals_on_host = bool(rng.random() < 0.3)
    t.slot = int(rng.integers(0, 4))
    t.mate_tags = bool(o.integers(0, 2))
    t.sam_seq = bool(o.integers(0, 2))
    t.estimate = [None, None, None, "first", "last"][int(o.integers(0, 5))]  # estimate_insert / _library: before the text, behind the BAM
    # the oracle's single-end records: what the models start from, and the inserts that occur
    t.ref = fo.Reference(seqs)
    t.idx = fo.OracleIndex(t.ref, threads=THREADS)
    t.se = cut_view(t).se  # (of the kept parts where a cut is on: the as-if property)
    # the insert range
    I = int([0, 0, max(L, L2), rng.integers(0, X // 2)][int(rng.integers(0, 4))])
    t.moved = None
    if t.paired and rng.random() < 0.6:  # a bound onto an insert that occurs: ins == X, ins == I
        ins = occurring_inserts(om.virtual(t.se, n, t.orientation), n)
        near = [v for v in ins if v <= 2000] or ins
        if near:
            v = int(near[int(rng.integers(0, len(near)))])
            if rng.integers(0, 2):
                if v >= I and v - I <= 65536:
                    X, t.moved = v, "X"
            elif 0 < v <= X:
                I, t.moved = v, "I"
    t.I, t.X = I, X
    assert 0 <= I <= X <= 1 << 30 and X - I <= 65536
    # XA: off, a limit of the ladder, or c - 1 of a slot that occurs, and that - 1 and + 1; with long names, in most trials one
    # name's length moved so that a prefix of some slot's entries has FEM_XA_MAX_BYTES bytes exactly, or one more
    t.xa = t.xa_moved = None
    u, v = o.random(), o.random()
    if u >= 0.25:
        t.xa = int(f.get("xa", XA_LIMITS[int(o.integers(0, len(XA_LIMITS)))]))
        seq = expected(t, full=False).seq  # (the text in front of the folding; the models' work is kept for the trial's own call)
        sizes = sorted({len(s) - 1 for s in xm.slots(seq) if len(s) > 1})  # (each size once: the large slots are few)
        if u >= 0.7 and sizes:
            t.xa = max(1, sizes[int(o.integers(0, len(sizes)))] + int(o.integers(-1, 2)))
        if t.long_names and v < 0.8:
            target = xm.MAX_BYTES + int(o.integers(0, 2))
            moves = budget_moves(seq, t.names, target)
            if moves:
                k, length, f = moves[int(o.integers(0, len(moves)))]
                t.names[k] = "chr%d_" % k + t.names[k][-1] * (length - len("chr%d_" % k))
                t.xa_moved = "B" if target == xm.MAX_BYTES else "B+1"
                if t.xa < f:
                    t.xa = xm.ALL
    if t.coverage:  # min_mapq: 0, or a MAPQ that occurs in the trial's text; without MAPQ the column is 255 and everything passes
        W, all_hits, min_mapq = t.coverage
        if cr.random() < 0.65:
            seen = sorted({int(l.split(b"\t", 5)[4]) for l in expected(t, full=False).seq.splitlines() if not int(l.split(b"\t", 2)[1]) & 4})
            # (... or one more than such a MAPQ, so that lines stand on either side of the bound)
            min_mapq = min(60, seen[int(cr.integers(0, len(seen)))] + int(cr.integers(0, 3) == 0)) if t.mapq and seen else int(cr.integers(0, 61))
        if t.cli and not t.mapq:  # (FEM map --coverage-mapq needs --mapq)
            min_mapq = 0
        t.coverage = (W, all_hits, min_mapq)
    return t


def draw_cuts(t, c, f, seqs, reads, quals, base):
    """The cut stage and the coverage track of a trial, drawn from `c` alone, and the world they need -> (seqs, reads, quals, the
    pairs' names).  t.trim (t5, t3, Q), t.adapter (A, A2 or None, O, E), t.overlap (O, E; paired trials only), t.coverage (W,
    all_hits, min_mapq; the last one is drawn at draw()'s end), each None where it is off; f: draw()'s force, which fixes each of
    the four on (True) or off (False).  With a cut on, cases.cut_pairs' pairs are appended (the reads a cut makes mappable, as the
    device is given them), every read's qualities come from trim_model's profiles, and nothing is staged packed: t.packed_first
    says that the trial stages packed first and expects the refusal.  t.records_first, t.again: with the track on, fem_dev_fetch_records
    precedes the text (and adds nothing); the slot's batch is mapped and fetched a second time (and the bins double)."""
    n, L, L2 = len(base), t.L, t.L2
    newer = c.random() < 0.55 or any(f.get(k) for k in ("trim", "adapter", "overlap", "coverage"))  # (by the clock: on in about half of the trials)

    def on(key):
        return bool(f[key]) if key in f else bool(newer and c.random() < 0.5)

    def fixed():
        return int(c.integers(0, 13)) if c.random() < 0.92 else int(c.integers(250, 1025))  # mostly small; sometimes more than a read

    t.trim = t.adapter = t.overlap = t.coverage = None
    if on("trim"):
        t.trim = (fixed(), fixed(), int(c.choice(TRIM_QUALS)))
        if t.trim == (0, 0, 0):
            t.trim = (0, 0, 20)
    if on("adapter"):
        lengths = adm.ADAPTERS + adm.ADAPTERS[1:]  # (the shortest one, which matches all over a read, half as often)
        m = int(c.choice(lengths))
        m2 = None if c.random() < 0.4 else int(c.choice(lengths))
        t.adapter = (util.rand_seq(c, m), None if m2 is None else util.rand_seq(c, m2), int(c.integers(1, min(m, m2 or m) + 1)), int(c.integers(0, 31)))
    if on("overlap") and t.paired:
        lo, low = 37 + 12 * t.e, min(L, L2)  # (O a fragment length that maps: cut_pairs makes a pair of f = o = O, where O + 1 must show)
        mappable = int(c.integers(lo, max(low, lo + 1)))
        t.overlap = (int([8, 20, c.integers(8, 61), c.integers(8, 61), c.integers(8, 61), c.integers(8, 1025), mappable, mappable][int(c.integers(0, 8))]),
                     int(c.integers(0, 31)))
    t.packed_first = False
    made = []  # (read, the foreign bases at its 3' end) of the reads made to be cut
    if t.trim or t.adapter or t.overlap:
        A, A2, aO, aE = t.adapter or (None, None, adm.O, adm.E)
        vO, vE = t.overlap or (None, ovm.E)
        flips = om.FLIPS[t.orientation] if t.paired else (0, 0)
        cp = cut_pairs(c, seqs, L, L2, t.e, flips, *(t.trim or (0, 0, 0)), A, A2, aO, aE, vO, vE, n=int(c.integers(3, 7)))
        k = len(cp["r1"])
        quals = [trm.profile_quals(c, CUT_PROFILES[int(c.integers(0, len(CUT_PROFILES)))], len(r), int(c.integers(0, 4))).decode("latin-1")
                 for r in reads]
        reads, quals = reads[:n] + cp["r1"] + reads[n:] + cp["r2"], quals[:n] + cp["q1"] + quals[n:] + cp["q2"]
        made = [(n + i, ta) for i, (ta, _) in enumerate(cp["tails"])] + [(2 * n + k + i, tb) for i, (_, tb) in enumerate(cp["tails"])]
        base = base + [_qname(c) for _ in range(k)]
        seqs = seqs + ([cp["seq"]] if cp["seq"] else [])
        t.packed_first, t.packed = t.packed, False
    t.made = [(r, tail) for r, tail in made if tail > 0]
    t.records_first = t.again = False
    if on("coverage"):
        lens = [len(s) for s in seqs]
        ladder = COVERAGE_WINDOWS + (max(lens) + 1, lens[int(c.integers(0, len(lens)))])
        t.coverage = (int(ladder[int(c.integers(0, len(ladder)))]), bool(c.integers(0, 2)), 0)
        t.records_first, t.again = bool(c.random() < 0.3), bool(c.random() < 0.3)
    return seqs, reads, quals, base


def batch_clips(t, trim, adapter, overlap):
    """([(c5, c3)], [a3] or None, [v3] or None) of the trial's reads as the device is given them, under these settings of the cut
    stage: overlap_model's composition for pairs, adapter_model's (which is trim_model's without an adapter) otherwise."""
    t5, t3, Q = trim or (0, 0, 0)
    A, A2, aO, aE = adapter or (None, None, adm.O, adm.E)
    if t.paired and overlap:
        cl, v3, a3 = ovm.batch_clips(t.reads, t.quals, t5, t3, Q, overlap[0], overlap[1], A=A, A2=A2, aO=aO, aE=aE, frag=ovm.frag_np)
    else:
        (cl, a3), v3 = adm.batch_clips(t.reads, t.quals, t5, t3, Q, A, aO, aE, A2, paired=t.paired), None
    return cl, a3 if adapter else None, v3


def cut_view(t, trim=_KEEP, adapter=_KEEP, overlap=_KEEP, tag=None, clips=None):
    """What the stages of expected() see of the batch under these settings of the cut stage (by default the trial's): .on, .clips,
    .a3, .v3 (None where the producer is off), .reads and .quals (the kept parts; the reads themselves with every cut off) and
    .se, the oracle's records of .reads.  Kept per trial and settings; tag: the name of a variant of the rule in that memo, clips:
    its (clips, a3, v3) (tests/test_fuzz_lines_model.py).  Settings that cut as the trial's own do are the trial's own view."""
    trim, adapter, overlap = (getattr(t, k) if x is _KEEP else x for k, x in (("trim", trim), ("adapter", adapter), ("overlap", overlap)))
    key = (trim, adapter, overlap, tag)
    memo = t.__dict__.setdefault("_views", {})
    if key not in memo:
        v = types.SimpleNamespace(key=key, on=bool(trim or adapter or overlap), clips=None, a3=None, v3=None, reads=t.reads, quals=t.quals)
        if v.on:
            v.clips, v.a3, v.v3 = clips or batch_clips(t, trim, adapter, overlap)
            v.reads = [r[a:len(r) - b] for r, (a, b) in zip(t.reads, v.clips)]
            v.quals = [q[a:len(q) - b] for q, (a, b) in zip(t.quals, v.clips)]
        own = memo.get((t.trim, t.adapter, t.overlap, None))
        if own is not None and (v.on, v.clips, v.a3, v.v3) == (own.on, own.clips, own.a3, own.v3):
            v = own
        else:
            v.se = fo.map_reads(t.ref, t.idx, fo.ReadBatch(v.reads), e=t.e, threads=THREADS)
        memo[key] = v
    return memo[key]


def budget_moves(seq, names, target):
    """Where one reference name's length can go so that a prefix of a slot's XA entries has `target` bytes: [(the name's index, its
    new length, the prefix's entries)] over the slots of `seq`, the text in front of the folding.  An entry's length is its RNAME's
    plus what the other columns take, so the first f entries, c of them on name k, reach the target iff c divides what is missing."""
    raw, out = [x.encode() for x in names], []
    for slot in xm.slots(seq):
        lens = [len(xm.entry(l)) for l in slot[1:]]
        on = [l.split(b"\t", 3)[2] for l in slot[1:]]
        for name in sorted(set(on)):
            k, total, c = raw.index(name), 0, 0
            for f in range(1, len(lens) + 1):
                total, c = total + lens[f - 1], c + (on[f - 1] == name)
                if c and (target - total) % c == 0 and 8 <= len(name) + (target - total) // c <= 254:
                    out.append((k, len(name) + (target - total) // c, f))
    return out


def options(t):
    return {k: getattr(t, k) for k in OPTIONS}


def fingerprint(t):
    """Everything draw() decided, in a form that compares."""
    return (repr(options(t)), tuple(t.seqs), tuple(t.reads), tuple(t.rnames), tuple(t.quals), tuple(t.names))


def rescued_lists(t, E=None, I=None, X=None, orientation=None, view=None):
    """(the virtual lists pairing sees, {read: its kept rescue}, {pair: every traced rescue}, {read: (kind, d)}) of a paired trial
    (orient_model.rescued: the rescue models on the virtual batch; under FR that is the batch itself).  view: the cut_view."""
    E, I, X = t.E if E is None else E, t.I if I is None else I, t.X if X is None else X
    orientation = t.orientation if orientation is None else orientation
    v = cut_view(t) if view is None else view
    memo = t.__dict__.setdefault("_rescued", {})
    key = (E, I, X, orientation, rm.ANCHORS, v.key)
    if key in memo:
        return memo[key]
    if t.rescue:
        out = om.rescued(v.se, t.n, v.reads, t.seqs, E, I, X, orientation, t.discordant)
    else:
        out = om.virtual(v.se, t.n, orientation), {}, {}, {}
    memo[key] = out
    return out


def lines_behind(t, w, xa=_KEEP, xa_bytes=xm.MAX_BYTES, view=None):
    """The stages behind w.plain, in the header's order, into w: tagged (RG, NH, HI), mated (MC, MQ, ms; pair mode only), with a
    cut on the clip stage (trim_model.apply on w.line_reads: the kept parts' text into the trimmed batch's), seq (SEQ and QUAL as
    SAM orders them: with a cut on that is the clip stage's own turn of the whole read), text (XA folded at `xa` entries and
    `xa_bytes` bytes, which count the clips) and n_xa, its entries."""
    xa = t.xa if xa is _KEEP else xa
    v = cut_view(t) if view is None else view
    w.tagged = tm.apply(w.plain, t.rg, t.hits)
    w.mated = mt.apply(w.tagged, t.n, v.quals) if t.paired and t.mate_tags else w.tagged
    if v.on:
        w.seq = trm.apply(w.mated, t.reads, t.quals, v.clips, t.rnames, paired=t.paired, sam_seq=t.sam_seq, line_reads=w.line_reads)
    else:
        w.seq = ss.apply(w.mated) if t.sam_seq else w.mated
    w.text, w.n_xa = (w.seq, 0) if xa is None else xm.apply(w.seq, xa, xa_bytes)
    return w


def track(t, w, window=None, all_hits=None, min_mapq=None):
    """The coverage track of the trial's expected text (coverage_model.bins).  A folded line's MAPQ is not in an entry, so with
    all_hits and min_mapq > 0 the text in front of the folding is read: folding never changes the track."""
    W, a, q = (x if y is None else y for x, y in zip(t.coverage, (window, all_hits, min_mapq)))
    text = w.seq if a and q > 0 else w.text
    return cvm.bins(text, t.names, [len(s) for s in t.seqs], W, a, q)


def expected(t, full=True, E=None, I=None, X=None, strata=_KEEP, max_hits=_KEEP, mapq_e=None, orientation=None, view=None):
    """The models' answer, composed in the order include/fem_hip.h states: the oracle's records, virtual under the orientation,
    through the rescue models; pairing, MAPQ, the unmapped reads' lines and the filter (report_model: w.virtual); the real strands
    (orient_model.real_text: w.plain); then lines_behind's stages.  w.counts: proper, rescued, rescued discordant, unmapped,
    filtered (the pair counts None single-end) and the XA entries.  With `full` also the fem_batch_pairs arrays, the BAM payload
    and, where the trial asks for them, the two estimates.  The keyword arguments replace one parameter of the rule
    (tests/test_fuzz_lines_model.py: an off-by-one must show).  The stages up to w.plain are kept per trial and parameter set.
    With a cut on (view: cut_view's, by default the trial's) every stage up to the mate tags runs on the kept parts, the as-if
    property of include/fem_hip.h; w.counts gains the trimmed reads and bases, the reads with adapter and their bases, the pairs
    with an overlap cut and their bases (0 where the producer is off); w.clips, w.a3, w.v3 are the view's, and w.bins the track
    of the expected text where the trial keeps one."""
    v = cut_view(t) if view is None else view
    se, reads, quals = v.se, v.reads, v.quals
    I, X = t.I if I is None else I, t.X if X is None else X
    strata = t.strata if strata is _KEEP else strata
    max_hits = t.max_hits if max_hits is _KEEP else max_hits
    orientation = t.orientation if orientation is None else orientation
    e = (t.e if mapq_e is None else mapq_e) if t.mapq else None
    memo = t.__dict__.setdefault("_plain", {})
    key = (E, I, X, strata, max_hits, e, orientation, tuple(t.names), rm.ANCHORS, v.key)
    if key in memo:
        w = types.SimpleNamespace(**memo[key])
    else:
        w = types.SimpleNamespace(pairs=None)  # (line_reads: every line's read, which the clip stage needs: the names repeat)
        if t.paired:
            ext, kept, traced, kinds = rescued_lists(t, E, I, X, orientation, v)
            w.virtual, dropped, w.line_reads = rp.paired(om.virtual(se, t.n, orientation), t.n, t.names, reads, t.rnames, quals, I, X, res=ext,
                                                rescued=set(kept), e=e, unmapped=t.unmapped, strata=strata, max_hits=max_hits, with_reads=True)
            w.plain = om.real_text(w.virtual, orientation)
            w.ext, w.kept, w.traced, w.kinds = ext, kept, traced, kinds
            n_unm = len(um.unmapped_reads(ext, 2 * t.n)) if t.unmapped else 0
            w.five = (pm.expected(ext, t.n, I, X)[1], len(kept), sum(k == 2 for k, _ in kinds.values()), n_unm, dropped)
        else:
            w.plain, dropped, w.line_reads = rp.single_end(se, t.names, reads, t.rnames, quals, e=e, unmapped=t.unmapped, strata=strata,
                                                  max_hits=max_hits, with_reads=True)
            w.five = (None, None, None, len(um.unmapped_reads(se, 2 * t.n)) if t.unmapped else 0, dropped)
        memo[key] = dict(w.__dict__)
    lines_behind(t, w, view=v)
    w.clips, w.a3, w.v3 = v.clips, v.a3, v.v3
    w.counts = w.five + (w.n_xa,) + (trm.counts(v.clips) if v.on else (0, 0)) + (adm.counts(v.a3) if v.a3 else (0, 0)) + \
        (ovm.counts(v.v3) if v.v3 else (0, 0))
    w.bins = track(t, w) if t.coverage else None
    if full:
        if t.paired:
            w.pairs = om.pair_arrays(se, t.n, I, X, orientation, ext=w.ext)
            if t.estimate:
                w.library, w.insert = om.library_estimate(se, t.n), om.estimate(se, t.n, orientation)
        w.bam = bam_payload(w.text, [x.encode() for x in t.names])
    return w


def bam_payload(text, ref_names):
    """The BAM records of a text with every tag: mate_tags_model's record of each line without XA (tags_model's behind
    bam_model's, MC MQ ms behind those), and XA of type Z as the last aux field."""
    bare, xa = [], []
    for l in text.splitlines():
        v = xm.xa_of(l)
        xa.append(v)
        bare.append((l if v is None else l[:len(l) - len(v) - 6]) + b"\n")
    out = []
    for rec, v in zip(bm.records(mt.bam_payload(b"".join(bare), ref_names)), xa):
        extra = b"" if v is None else b"XAZ" + v + b"\0"
        out.append(struct.pack("<i", len(rec) - 4 + len(extra)) + rec[4:] + extra)
    return b"".join(out)


# the slice of tests/test_gpu_fuzz_lines.py, which tests/test_fuzz_lines_model.py holds to its conditions:
# id, seed, trials, force, the trials that also go through the command line
NO_CUTS = {"trim": False, "adapter": False, "overlap": False, "coverage": False}  # the cases from before the cut stage and the track were drawn
CUTS = {"trim": True, "adapter": True, "overlap": True}
SLICE = [("single-end-heavy", 18, 12, dict(NO_CUTS, single_end=0.6), ()), ("copies-80", 15, 12, dict(NO_CUTS, copies=80), ()),
         ("e-7", 25, 12, dict(NO_CUTS, e=7), ()), ("command-line", 21, 12, dict(NO_CUTS), (3,)),
         ("long-names", 24, 12, dict(NO_CUTS, long_names=True, copies=80), ()),
         ("xa-deep", 16, 12, dict(NO_CUTS, copies=200, strata=None, max_hits=None, xa=xm.ALL), ()),
         ("cuts", 67, 12, dict(CUTS), ()), ("cuts-pairs", 63, 12, dict(CUTS, paired=True), ()),
         ("coverage", 49, 12, {"coverage": True}, ()), ("cuts-command-line", 59, 12, {"adapter": True, "overlap": True, "cli_force": {"trim": True, "coverage": True, "mapq": True}}, (0,))]


def trial_force(force, cli):
    """draw()'s force of a trial: one that goes through the command line is paired and made for FASTQ files."""
    force = dict(force or {})
    only_cli = force.pop("cli_force", {})  # (what a case fixes for its command-line trials alone)
    return dict(force, cli=True, paired=True, **only_cli) if cli else force


def draw_cli(t, seed, k):
    """What a command-line trial draws besides draw(): t.bam, and t.batch, FEM map's --batch: an even number below the trial's n
    pairs, so the files take several batches and the track sums over them."""
    rng = np.random.default_rng([seed, k, 1])
    t.bam = bool(rng.integers(0, 2))
    t.batch = 2 * int(rng.integers(1, max(2, t.n // 2)))


def slice_trials():
    """(seed, k, force) of every trial of SLICE."""
    return [(seed, k, trial_force(force, k in cli)) for _, seed, trials, force, cli in SLICE for k in range(trials)]


# ---- the device ----

def _counts(dev, t):
    from fem_amd import FemError
    out = []
    for count in (dev.pair_count, dev.rescue_count, dev.rescue_discordant_count):
        try:
            out.append(count(slot=t.slot))
        except FemError as err:  # single-end: the three pair counts refuse
            if t.paired or "the slot is not in pair mode" not in str(err):
                raise
            out.append(None)
    return tuple(out) + (dev.unmapped_count(slot=t.slot), dev.filtered_count(slot=t.slot), dev.xa_count(slot=t.slot)) + \
        dev.trim_count(slot=t.slot) + dev.adapter_count(slot=t.slot) + dev.pair_overlap_count(slot=t.slot)


def set_options(dev, t, X=None, trim5=None):
    """Every option of the trial's slot through its own setter, the ones that go off included: what the slot's last trial left of
    a cut meets a trial without one."""
    s = t.slot
    t5, t3, Q = t.trim or (0, 0, 0)
    dev.set_trim(t5 if trim5 is None else trim5, t3, Q, slot=s)
    dev.set_adapter(*(t.adapter or (None,)), slot=s)
    dev.set_pair_overlap(*(t.overlap or (None,)), slot=s)
    dev.set_pairs(t.I, t.X if X is None else X, slot=s) if t.paired else dev.set_pairs(None, slot=s)
    dev.set_rescue(t.E if t.rescue else None, slot=s)
    dev.set_rescue_discordant(t.discordant, slot=s)
    dev.set_mapq(t.mapq, slot=s)
    dev.set_unmapped(t.unmapped, slot=s)
    dev.set_report(strata=t.strata, max_hits=t.max_hits, slot=s)
    dev.set_tags(slot=s, read_group=t.rg, hits=t.hits)
    dev.set_orientation(t.orientation, slot=s)  # (single-end too: it must change nothing there, nor must the mate tags)
    dev.set_mate_tags(t.mate_tags, slot=s)
    dev.set_sam_seq(t.sam_seq, slot=s)
    dev.set_xa(0 if t.xa is None else t.xa, slot=s)


def _estimates(dev, t, want, when, diffs):
    """estimate_insert and estimate_library of the trial's slot against the models."""
    got = dev.estimate_insert(slot=t.slot).as_tuple()
    if got != im.as_tuple(want.insert):
        diffs.append("estimate_insert %s: got %r want %r" % (when, got, im.as_tuple(want.insert)))
    lib = dev.estimate_library(slot=t.slot)
    got, model = ([e.as_tuple() for e in lib.by], lib.orientation), ([im.as_tuple(e) for e in want.library["by"]], want.library["orientation"])
    if got != model:
        diffs.append("estimate_library %s: got %r want %r" % (when, got, model))


def _refused(call, words, what, diffs):
    """call() must be refused by the device layer with one of `words` in the message; anything else it raises is raised."""
    from fem_amd import FemError
    try:
        call()
        diffs.append(what)
    except FemError as err:
        if not any(x in str(err) for x in words):
            raise


def _cuts(dev, t, want, diffs):
    """The clip points and each producer's cuts of the slot's batch, read for read, against the models'."""
    s = t.slot
    for what, fetch, model in (("fetch_trim", dev.fetch_trim, want.clips and list(zip(*want.clips))), ("fetch_adapter", dev.fetch_adapter, want.a3 and [want.a3]),
                               ("fetch_pair_overlap", dev.fetch_pair_overlap, want.v3 and [want.v3])):
        if model is None:
            _refused(lambda: fetch(slot=s), ("was mapped without",), "%s: not refused for a batch mapped without it" % what, diffs)
            continue
        got = fetch(slot=s)
        got = list(got) if isinstance(got, tuple) else [got]
        for g, m in zip(got, model or [[]] * len(got)):
            if [int(x) for x in g] != list(m):
                bad = next((i for i, (a, b) in enumerate(zip(g, m)) if int(a) != b), min(len(g), len(m)))
                diffs.append("%s: read %d of %d (model: %d reads)" % (what, bad, len(g), len(m)))
                break


def _track(dev, bins, what, diffs):
    got = dev.fetch_coverage()
    if not np.array_equal(got, bins):
        bad = np.flatnonzero(got != bins) if len(got) == len(bins) else []
        diffs.append("%s: %d bins, the model %d" % (what, len(got), len(bins)) if len(got) != len(bins) else
                     "%s: %d bins differ, the first one %d: got %d want %d" % (what, len(bad), bad[0], got[bad[0]], bins[bad[0]]))


def compare(dev, t, want, X=None, trim5=None):
    """The device on the trial -> the list of differences (empty: everything compared is identical).  An error of the device layer
    is raised, not listed.  X, trim5: the device's max_insert and trim5, if not the trial's (to show that a difference is seen)."""
    from fem_amd import device
    s, diffs = t.slot, []
    cut_on = bool(t.trim or t.adapter or t.overlap)
    dev.upload_reference(t.seqs)
    dev.upload_reference_names(t.names)
    dev.upload_index(12, 3, t.idx.lookup, t.idx.occ[:t.idx.n_occ])
    set_options(dev, t, X, trim5)
    dev.set_coverage(*(t.coverage or (None,)))  # (behind upload_reference, which turns the track off)
    batch = fo.ReadBatch(t.reads)
    q = np.frombuffer("".join(t.quals).encode("latin-1"), np.uint8)
    if t.packed or t.packed_first:
        hb, _ = dev.acquire_stage(2 * t.n, 2 * t.n * t.L, slot=s)
        dev.commit_stage_packed(2 * t.n, t.L, device.pack_reads(batch.bases, 2 * t.n, t.L, hb), slot=s)
    if t.packed_first:  # a packed batch with a cut on: refused at the map, and staged as characters then
        dev.stage_text(q, t.rnames, slot=s)
        _refused(lambda: dev.map_staged(e=t.e, slot=s), ("input not supported by the device path",), "map_staged: a packed batch with a cut on", diffs)
    if not t.packed:
        dev.stage_reads(batch.bases, batch.off, slot=s)
    if dev.stage_info(s)[1] != t.packed and (t.packed or cut_on):  # (with a cut on, reads of one length go as characters too)
        diffs.append("staging: packed with a cut on" if not t.packed else "staging: not packed")
    dev.stage_text(q, t.rnames, slot=s, quals_on_host=t.quals_on_host)
    on_host = t.quals_on_host
    if on_host and t.trim and t.trim[2] > 0:  # the quality rule reads the qualities on the device, in front of the mapping
        _refused(lambda: dev.map_staged(e=t.e, slot=s), ("quality trimming",), "map_staged: --trim-qual with the qualities on the host", diffs)
        dev.stage_text(q, t.rnames, slot=s)
        on_host = False
    dev.map_staged(e=t.e, slot=s)
    hq = dict(quals=q, offsets=batch.off) if on_host else {}
    if t.records_first:  # (with the track on: it adds nothing)
        dev.fetch_records(slot=s)
    if t.estimate == "first" and t.paired:  # (the header's promise: what is fetched afterwards is what it is without the calls)
        _estimates(dev, t, want, "before the text", diffs)
    # QUAL reversed, ms:i and a trimmed batch's QUAL are made from the qualities on the device: with them on the host the text is
    # refused, and only there
    refuses = t.sam_seq or (t.paired and t.mate_tags) or cut_on
    if on_host and refuses:
        _refused(lambda: dev.fetch_sam(slot=s, nowait=t.nowait, **hq), ("qualities", "a trimmed batch"), "fetch_sam: a text with the qualities on the host", diffs)
        dev.stage_text(q, t.rnames, slot=s)
        on_host, hq = False, {}
    # the text, the counts behind it, the text again the other way
    text, _, _, stats = dev.fetch_sam(slot=s, nowait=t.nowait, **hq)
    if text != want.text:
        diffs.append("fetch_sam: " + first_difference(text, want.text))
    got = _counts(dev, t)
    if got != want.counts:
        diffs.append("counts after the text: got %r want %r" % (got, want.counts))
    again = dev.fetch_sam(slot=s, nowait=not t.nowait, **hq)[0]
    if again != text:
        diffs.append("fetch_sam, the other nowait: " + first_difference(again, text))
    if dev.xa_count(slot=s) != want.counts[5]:
        diffs.append("xa_count after the text, the other nowait: got %d want %d" % (dev.xa_count(slot=s), want.counts[5]))
    # BAM at the drawn level (its qualities on the device)
    if on_host:
        dev.stage_text(q, t.rnames, slot=s)
    data = dev.fetch_bam(slot=s, level=t.bam_level, nowait=t.nowait)
    members = [m[0] for m in bm.parse_bgzf(data[0], eof=False)] if data[0] else []
    payload = b"".join(members)
    if payload != want.bam:
        ref_names = [x.encode() for x in t.names]
        try:
            where = first_difference(bm.bam_payload_to_sam(payload, ref_names), bm.bam_payload_to_sam(want.bam, ref_names))
        except Exception as err:  # (records that do not decode)
            where = "undecodable: %r" % err
        diffs.append("fetch_bam level %d: %s" % (t.bam_level, where))
    if data[1] != len(payload):
        diffs.append("fetch_bam: raw_len %d, %d bytes in the members" % (data[1], len(payload)))
    if (gzip.decompress(data[0]) if data[0] else b"") != payload:
        diffs.append("fetch_bam: gzip inflates to other bytes")
    try:
        for m in members:
            bm.records(m)
    except Exception:
        diffs.append("fetch_bam: a record spans two members")
    got = _counts(dev, t)
    if got != want.counts:
        diffs.append("counts after the BAM: got %r want %r" % (got, want.counts))
    if dev.fetch_bam(slot=s, level=t.bam_level, nowait=not t.nowait)[0] != data[0]:
        diffs.append("fetch_bam, the other nowait: other bytes")
    if dev.xa_count(slot=s) != want.counts[5]:
        diffs.append("xa_count after the BAM, the other nowait: got %d want %d" % (dev.xa_count(slot=s), want.counts[5]))
    if t.estimate == "last" and t.paired:  # ... and behind the BAM: the text, the BAM and the counts after them are as before
        _estimates(dev, t, want, "behind the BAM", diffs)
        if dev.fetch_sam(slot=s, nowait=t.nowait)[0] != text or _counts(dev, t) != want.counts:
            diffs.append("behind the estimates: another text or other counts")
        if dev.fetch_bam(slot=s, level=t.bam_level, nowait=t.nowait)[0] != data[0] or _counts(dev, t) != want.counts:
            diffs.append("behind the estimates: another BAM or other counts")
    # fem_batch_pairs; fem_batch_records and the stats keep their single-end meaning
    if t.paired:
        pairs = dev.fetch_pairs(slot=s)
        for k, v in want.pairs.items():
            g = getattr(pairs, k)
            if not (g == v if k == "n_proper" else np.array_equal(g, v)):
                diffs.append("fetch_pairs: %s differs" % k)
                break
    _cuts(dev, t, want, diffs)
    if t.coverage:  # the track: the batch added exactly once by all the fetches above
        if refuses:  # ... and not by a refused one
            dev.stage_text(q, t.rnames, slot=s, quals_on_host=True)
            _refused(lambda: dev.fetch_sam(slot=s, quals=q, offsets=batch.off), ("qualities", "a trimmed batch"), "fetch_sam: a text with the qualities on the host, behind the BAM", diffs)
            dev.stage_text(q, t.rnames, slot=s)
        _track(dev, want.bins, "the track", diffs)
        if t.again:  # the slot's batch mapped and fetched a second time: exactly doubled
            dev.stage_reads(batch.bases, batch.off, slot=s)
            dev.stage_text(q, t.rnames, slot=s)
            dev.map_staged(e=t.e, slot=s)
            if dev.fetch_sam(slot=s, nowait=t.nowait)[0] != text:
                diffs.append("fetch_sam of the batch mapped again: another text")
            _track(dev, 2 * want.bins, "the track after the batch was mapped and fetched again", diffs)
    se, rec = t.se, dev.fetch_records(slot=s)
    for k, g, v in (("rec_begin", rec.rec_begin, se.rec_off), ("flag", rec.flag & 0x7FFF, se.r_flag & 0x7FFF), ("pos0", rec.pos0, se.r_pos),
                    ("tid", rec.tid, se.r_tid), ("nm", rec.nm, se.r_nm), ("cigar_off", rec.cigar_off, se.cig_off), ("cigar", rec.cigar, se.cig),
                    ("md_off", rec.md_off, se.md_off), ("md", rec.md, se.md), ("stats", stats, se.stats), ("stats", rec.stats, se.stats)):
        if not np.array_equal(g, v):
            diffs.append("fetch_records: %s differs" % k)
            break
    return diffs


# ---- FEM index + FEM map ----

def _counters(t, want):
    st = [int(x) for x in t.se.stats]
    out = ["The number of read: %d" % st[0], "The number of mapped read: %d" % st[1],
           "The number of candidate before additional q-gram filter: %d" % st[2], "The number of candidate: %d" % st[3],
           "The number of mapping: %d" % st[4], "The number of proper pairs: %d" % want.counts[0]]
    if t.rescue:
        out.append("The number of rescued mates: %d" % want.counts[1])
        if t.discordant:
            out.append("The number of rescued discordant pairs: %d" % want.counts[2])
    if t.unmapped:
        out.append("The number of unmapped reads: %d" % want.counts[3])
    if t.strata is not None or t.max_hits is not None:
        out.append("The number of filtered lines: %d" % want.counts[4])
    if t.xa is not None:
        out.append("The number of XA entries: %d" % want.counts[5])
    if t.trim or t.adapter or t.overlap:
        out += ["The number of trimmed reads: %d" % want.counts[6], "The number of trimmed bases: %d" % want.counts[7]]
    if t.adapter:
        out += ["The number of reads with adapter: %d" % want.counts[8], "The number of adapter bases: %d" % want.counts[9]]
    if t.overlap:
        out += ["The number of pairs with overlap cut: %d" % want.counts[10], "The number of overlap bases: %d" % want.counts[11]]
    if t.coverage:
        out.append("The number of covered bases: %d" % int(want.bins.sum()))
    return out


def compare_cli(t, want, timeout=300):
    """The paired trial through FEM index + FEM map with the drawn switches -> the list of differences."""
    diffs = []
    with tempfile.TemporaryDirectory() as tmp:
        fa, idx_path, out = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref.idx"), os.path.join(tmp, "out")
        with open(fa, "wb") as fh:
            fh.write(b"".join(b">" + nm.encode() + b" desc\n" + s + b"\n" for nm, s in zip(t.names, t.seqs)))
        build_index(fa, idx_path)
        n = t.n
        paths = [pathlib.Path(tmp) / "r1.fq", pathlib.Path(tmp) / "r2.fq"]
        for m, suffix in ((0, "/1"), (1, "/2")):
            write_fastq(paths[m], t.reads[m * n:(m + 1) * n], [x + suffix for x in t.rnames[m * n:(m + 1) * n]],
                         t.quals[m * n:(m + 1) * n], False)
        args = ["-e", str(t.e), "-t", "4", "--ref", fa, "--index", idx_path, "--read1", str(paths[0]), "--read2", str(paths[1]),
                "-o", out, "--batch", str(t.batch), "-I", str(t.I), "-X", str(t.X)]
        if t.rescue:
            args += ["--rescue", str(t.E)] + (["--rescue-discordant"] if t.discordant else [])
        args += (["--mapq"] if t.mapq else []) + (["--unmapped"] if t.unmapped else []) + (["--nh"] if t.hits else [])
        args += ([] if t.strata is None else ["--strata", str(t.strata)]) + ([] if t.max_hits is None else ["--max-hits", str(t.max_hits)])
        args += [] if t.rg is None else ["--rg", "@RG\tID:" + t.rg.decode("latin-1")]
        args += ["--orientation", om.NAMES[t.orientation]] + (["--mate-tags"] if t.mate_tags else []) + (["--sam-seq"] if t.sam_seq else [])
        args += [] if t.xa is None else ["--xa"] if t.xa == xm.ALL else ["--xa=%d" % t.xa]
        if t.trim:  # (--trim-qual 0 is refused: the quality rule is off without the switch)
            args += ["--trim5", str(t.trim[0]), "--trim3", str(t.trim[1])] + (["--trim-qual", str(t.trim[2])] if t.trim[2] else [])
        if t.adapter:
            A, A2, aO, aE = t.adapter
            args += ["--adapter", A.decode()] + ([] if A2 is None else ["--adapter2", A2.decode()]) + ["--adapter-overlap", str(aO), "--adapter-err", str(aE)]
        if t.overlap:
            args += ["--trim-overlap", "--trim-overlap-min", str(t.overlap[0]), "--trim-overlap-err", str(t.overlap[1])]
        if t.coverage:  # the track sums over the batches of the run
            W, all_hits, min_mapq = t.coverage
            bed = os.path.join(tmp, "track.bed")
            args += ["--coverage", bed, "--coverage-window", str(W)] + (["--coverage-all"] if all_hits else [])
            args += ["--coverage-mapq", str(min_mapq)] if min_mapq else []
        args += ["--bam=%d" % t.bam_level] if t.bam else []
        r = run_fem("map", *args, timeout=timeout)
        if r.returncode != 0:
            return ["FEM map: exit status %d: %s" % (r.returncode, r.stderr.decode("latin-1")[-400:])]
        data = decode_bam_file(out) if t.bam else open(out, "rb").read()
        lines = data.split(b"\n")
        k = next((i for i, l in enumerate(lines) if not l.startswith(b"@")), len(lines))
        body = b"\n".join(lines[k:])
        if body != want.text:
            diffs.append("FEM map%s: %s" % (" --bam" if t.bam else "", first_difference(body, want.text)))
        got = [l for l in r.stderr.decode("latin-1").splitlines() if l.startswith("The number of")]
        if got != _counters(t, want):
            diffs.append("FEM map: counters %r want %r" % (got, _counters(t, want)))
        if t.coverage:
            got, model = open(bed, "rb").read(), cvm.bed(t.names, [len(x) for x in t.seqs], t.coverage[0], want.bins)
            if got != model:
                diffs.append("FEM map --coverage: " + first_difference(got, model))
    return diffs


# ---- the run ----

def run_trial(dev, seed, k, force=None, cli=False, log=print, **device):
    """Trial k of `seed` -> True if everything compared is identical.  device: compare()'s X or trim5, the device's setting where
    it is not to be the trial's."""
    t = draw(np.random.default_rng([seed, k]), trial_force(force, cli))
    want = expected(t)
    diffs = compare(dev, t, want, **device)
    if cli:
        draw_cli(t, seed, k)
        diffs += compare_cli(t, want)
    log("seed %d trial %d" % (seed, k), options(t), "lines %d" % want.text.count(b"\n"), "counts %r" % (want.counts,),
        "ok" if not diffs else "MISMATCH: " + "; ".join(diffs))
    return not diffs


def run(seed, trials=None, seconds=None, log=print, force=None, cli_trials=None, only=None):
    """`trials` trials of `seed` (0 .. trials - 1), or trials for `seconds`; only: that one trial alone -> (n_trials, bad).
    force: draw()'s.  cli_trials: the trials that are paired and also go through the command line; by default every sixth trial
    of a run by the clock (a rule on k alone, so that FUZZ_TRIAL meets the same trial).  A mismatch is logged and counted; an
    error of the device layer ends the run: it is raised, and nothing more is started on the GPU."""
    from fem_amd import Device
    t_end = time.time() + seconds if seconds else None
    n_trials = bad = 0
    dev = Device(0)
    for k in itertools.count() if only is None else [only]:
        if only is None and (time.time() >= t_end if t_end else k >= trials):
            break
        cli = k in cli_trials if cli_trials is not None else bool(t_end) and k % 6 == 5
        n_trials += 1
        bad += not run_trial(dev, seed, k, force, cli, log)
    dev.close()
    return n_trials, bad


if __name__ == "__main__":
    only = os.environ.get("FUZZ_TRIAL")
    n_trials, bad = run(int(os.environ.get("FUZZ_SEED", "1")), seconds=float(os.environ.get("FUZZ_SECONDS", "240")),
                        only=None if only is None else int(only))
    print("trials", n_trials, "bad", bad)
    sys.exit(1 if bad else 0)
