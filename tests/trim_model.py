"""Read trimming (fem_dev_set_trim, FEM map --trim5 / --trim3 / --trim-qual), the rule in plain Python.
clips() is the serial rule of include/fem_hip.h, kept() the kept parts of a batch, apply() turns the SAM text of the batch of the
kept parts into the text of the trimmed batch by the as-if differences: S operations around every CIGAR that is printed (the
CIGAR column, MC:Z, the entries of XA:Z), SEQ and QUAL of the whole read, ms:i over the other mate's whole qualities.  The
letter table is that of tests/sam_seq_model.py."""
import functools
import re

import numpy as np

from oracle import fem_oracle as fo
from tests import cases
from tests import util

MIN_KEEP = 35  # FEM_TRIM_MIN_KEEP

LETTERS = "=ACMGRSVTWYHKDBN"      # what a SAM line prints: the letter of 4-bit code 0, 1, .. 15
COMPLEMENT = "=TGKCYSBAWRDMHVN"   # ... and the complement of each
_COMP = {ord(a): ord(b) for a, b in zip(LETTERS, COMPLEMENT)}
MS_MIN_QUAL = 15


def printed(ch):
    """The letter a read character is printed as: IUPAC upper-cased, else N."""
    up = chr(ch).upper()
    return ord(up) if up in LETTERS else ord("N")


def clips(qual_bytes, t5, t3, Q):
    """(c5, c3) of a read with these quality bytes under --trim5 t5 --trim3 t3 --trim-qual Q (Q = 0: off)."""
    b = bytes(qual_bytes)
    L = len(b)
    c5 = min(t5, L)
    c3f = min(t3, L - c5)
    Lp = L - c5 - c3f
    cut = Lp
    if Q >= 1 and Lp > MIN_KEEP:
        s = best = 0
        for l in range(Lp - 1, MIN_KEEP - 1, -1):
            s += Q - (b[c5 + l] - 33)
            if s < 0:
                break
            if s > best:
                best, cut = s, l
    return c5, c3f + (Lp - cut)


def clips_parallel(qual_bytes, t5, t3, Q):
    """The same by the parallel form of the rule: suffix sums, the last negative one, the largest place of the maximum behind it."""
    b = bytes(qual_bytes)
    L = len(b)
    c5 = min(t5, L)
    c3f = min(t3, L - c5)
    Lp = L - c5 - c3f
    cut = Lp
    if Q >= 1 and Lp > MIN_KEEP:
        S = [0] * (Lp + 1)
        for l in range(Lp - 1, -1, -1):
            S[l] = S[l + 1] + Q - (b[c5 + l] - 33)
        stop = max([l for l in range(MIN_KEEP, Lp) if S[l] < 0], default=MIN_KEEP - 1)
        rng = range(stop + 1, Lp)
        top = max((S[l] for l in rng), default=0)
        if top > 0:
            cut = max(l for l in rng if S[l] == top)
    return c5, c3f + (Lp - cut)


def _bytes(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def batch_clips(quals, t5, t3, Q):
    """[(c5, c3)] of a batch's quality strings."""
    return [clips(_bytes(q), t5, t3, Q) for q in quals]


def counts(cl):
    """(reads with c5 + c3 > 0, the sum of c5 + c3): the two counters."""
    return sum(1 for a, b in cl if a + b), sum(a + b for a, b in cl)


def kept(reads, quals, t5, t3, Q):
    """-> (the kept parts of the reads, of the qualities, the clips)."""
    cl = batch_clips(quals, t5, t3, Q)
    cut = lambda x, c: x[c[0]:len(x) - c[1]]  # noqa: E731
    return [cut(r, c) for r, c in zip(reads, cl)], [cut(q, c) for q, c in zip(quals, cl)], cl


def clip_cigar(cigar, c5, c3, reverse):
    """A CIGAR column with the read's clips around it; * stays *."""
    if cigar == b"*":
        return cigar
    front, back = (c3, c5) if reverse else (c5, c3)
    return (b"%dS" % front if front else b"") + cigar + (b"%dS" % back if back else b"")


def ms_score(qual):
    return sum(b - 33 for b in _bytes(qual) if b - 33 >= MS_MIN_QUAL)


def apply(text, reads, quals, cl, rnames, paired=False, sam_seq=False, line_reads=None):
    """The SAM text (bytes, no header) of the trimmed batch from the text of the batch of the kept parts.  reads, quals: the whole
    reads; cl: their clips; rnames: the batch's read names, unique (pairs: the names of the n / 2 pairs; read i and n / 2 + i are
    the mates, told apart by 0x40 / 0x80).  line_reads: the read of every line, from the stage that made the lines
    (report_model, with_reads); the names may then repeat and are not looked at."""
    n = len(reads)
    half = n // 2
    lines = [l.split(b"\t") for l in text.split(b"\n") if l]
    if line_reads is None:
        index = {_bytes(nm): i for i, nm in enumerate(rnames)}
        assert len(index) == len(rnames)
        line_reads = [index[f[0]] + (half if paired and int(f[1]) & 0x80 else 0) for f in lines]
    assert len(line_reads) == len(lines)
    primary_rev = {}  # read -> its primary line's strand, for the MC of the other mate's lines
    for f, r in zip(lines, line_reads):
        flag = int(f[1])
        if not flag & 0x104:
            primary_rev.setdefault(r, bool(flag & 16))
    out = []
    for f, r in zip(lines, line_reads):
        flag = int(f[1])
        c5, c3 = cl[r]
        rev = bool(flag & 16)
        f[5] = clip_cigar(f[5], c5, c3, rev)
        if not flag & 0x100:  # the line carries SEQ and QUAL: the whole read as given
            seq = bytes(printed(c) for c in _bytes(reads[r]))
            qual = _bytes(quals[r])
            if sam_seq and rev:
                seq, qual = bytes(_COMP[c] for c in reversed(seq)), qual[::-1]
            f[9], f[10] = seq or b"*", qual or b"*"
        for k in range(11, len(f)):
            if f[k].startswith(b"MC:Z:"):
                o = r - half if r >= half else r + half
                f[k] = b"MC:Z:" + clip_cigar(f[k][5:], cl[o][0], cl[o][1], primary_rev[o])
            elif f[k].startswith(b"ms:i:"):
                o = r - half if r >= half else r + half
                f[k] = b"ms:i:%d" % ms_score(quals[o])
            elif f[k].startswith(b"XA:Z:"):
                ent = []
                for e in f[k][5:].split(b";")[:-1]:
                    rn, pos, cg, nm = e.rsplit(b",", 3)
                    ent.append(b",".join([rn, pos, clip_cigar(cg, c5, c3, pos[:1] == b"-"), nm]) + b";")
                f[k] = b"XA:Z:" + b"".join(ent)
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def clipped_reverse_lines(text):
    """The lines with 0x10 whose CIGAR carries an S operation."""
    return [l for l in text.split(b"\n") if l and int(l.split(b"\t", 2)[1]) & 16 and re.search(rb"\dS", l.split(b"\t")[5])]


# ---- cases of tests/test_gpu_trim.py ----

def tailed_reads(rng, seqs, n, L, e, max_tail=40, first=0):
    """n reads of L bases: a reference substring of L - t bases with 0..e substitutions, then t = 0..max_tail random bases; every
    second read reverse-complemented (its tail is then at its 5' end on the reference, still at the 3' end of the read).
    Qualities: the body I, the tail #, so that --trim-qual 20 cuts at the tail's start.  -> reads, quals, tails."""
    reads, quals, tails = [], [], []
    for i in range(n):
        t = int(rng.integers(0, max_tail + 1))
        si = int(rng.integers(0, len(seqs)))
        at = int(rng.integers(0, len(seqs[si]) - L))
        body = bytearray(seqs[si][at:at + L - t])
        if (first + i) % 2:
            body = bytearray(util.revcomp(bytes(body)))
        for p in rng.choice(len(body), int(rng.integers(0, e + 1)), replace=False):
            body[p] = b"ACGT"[(b"ACGT".index(bytes([body[p]]).upper()) + 1 + int(rng.integers(0, 3))) % 4] if bytes([body[p]]).upper() in b"ACGT" else 65
        reads.append(bytes(body) + util.rand_seq(rng, t))
        quals.append("I" * (L - t) + "#" * t)
        tails.append(t)
    return reads, quals, tails


@functools.lru_cache(maxsize=None)
def tails_case():
    """The issue's measured case: seed 5, a random reference of 300 kbp, 600 reads of 120 bases, e = 3, tails of 0..40."""
    rng = np.random.default_rng(5)
    seqs, names = [util.rand_seq(rng, 300_000)], ["chr0"]
    reads, quals, tails = tailed_reads(rng, seqs, 600, 120, 3)
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    return dict(seqs=seqs, names=names, reads=reads, quals=quals, tails=tails, rnames=["t%d" % i for i in range(len(reads))], e=3, ref=ref,
                idx=idx, trim=(0, 0, 20))


@functools.lru_cache(maxsize=None)
def ragged_case(repeats=False, seed=7, n=500):
    """Reads of 60..150 bases with tails on a reference with or without repeats, some odd ones among them: lower case, IUPAC
    letters, a read of length 0, reads at and below the floor of 35 bases, a read the fixed trims use up."""
    rng = np.random.default_rng(seed)
    seqs, names = cases.reference(rng, repeats)
    if repeats:  # long names: the XA entries of a slot reach the byte budget
        names = ["rich%d_" % i + "r" * 194 for i in range(3)] + ["exact_" + "e" * 54]
    reads, quals = [], []
    for i in range(n):
        r, q, _ = tailed_reads(rng, seqs, 1, int(rng.integers(60, 151)), 2, 30, first=i)
        reads += r
        quals += q
    reads[3] = reads[3].lower()
    reads[5] = reads[5][:20] + b"RYKM=.-*" + reads[5][28:]
    reads[7], quals[7] = b"", ""
    reads[9], quals[9] = reads[9][:35], quals[9][:35]
    reads[11], quals[11] = reads[11][:6], quals[11][:6]
    reads[13], quals[13] = reads[13][:36], "#" * 36
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    return dict(seqs=seqs, names=names, reads=reads, quals=quals, rnames=["g%d" % i for i in range(n)], e=3, ref=ref, idx=idx, trim=(3, 4, 20))


LENGTHS = (0, 1, 34, 35, 36, 37, 63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 1023, 1024)  # the floor and every chunk boundary
SETTINGS = ((0, 0, 20), (5, 0, 0), (0, 7, 0), (3, 4, 20), (1024, 0, 0), (60, 60, 2), (0, 0, 1), (0, 0, 93))
PROFILES = ("good", "bad", "illumina", "walk", "tail", "plateau", "low")


def profile_quals(rng, kind, L, k):
    """Quality bytes of one read of L bases; k varies the plateaus' level and the tail's length."""
    from tests import bam_model as bm
    if kind == "good":
        return b"I" * L
    if kind == "bad":
        return b"#" * L
    if kind == "illumina":
        return bm.illumina_quals(rng, L)
    if kind == "walk":
        return bm.random_walk_quals(rng, L)
    if kind == "tail":  # a bad tail with one good base in it
        t = min(L, 5 + 9 * k)
        q = bytearray(b"I" * (L - t) + b"#" * t)
        if t > 2:
            q[L - 1 - int(rng.integers(0, t - 1))] = ord("I")
        return bytes(q)
    if kind == "plateau":  # runs at q == Q for Q of 20, 2, 1, 93 between better and worse bases
        level = 33 + (20, 2, 1, 93)[k % 4]
        q = bytearray(rng.choice([level, level, level, 33 + 40, 33], size=L).astype(np.uint8))
        q[L // 2:L // 2 + 70] = bytes([level]) * len(q[L // 2:L // 2 + 70])
        return bytes(q)
    return bytes(rng.integers(0, 60, L).astype(np.uint8))  # "low": bytes below 33 among the others


@functools.lru_cache(maxsize=None)
def clip_case(per=16):
    """One ragged batch: every length of LENGTHS with every profile, `per` reads each (about 2 000 reads)."""
    rng = np.random.default_rng(11)
    reads, quals = [], []
    for L in LENGTHS:
        for kind in PROFILES:
            for k in range(per):
                reads.append(util.rand_seq(rng, L))
                quals.append(profile_quals(rng, kind, L, k).decode("latin-1"))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order], [quals[i] for i in order]
