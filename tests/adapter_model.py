"""3' adapter matching (fem_dev_set_adapter, FEM map --adapter), the rule in plain Python.  cut() is the serial
rule of include/fem_hip.h, cut_parallel() the same through per-window occurrence masks, the form adapter_match_kernel has;
clips() composes it with the fixed trims and the quality step of tests/trim_model.py.  The text of a batch trimmed this way is
trim_model.apply of the kept parts' text with these clips."""
import functools

import numpy as np

from oracle import fem_oracle as fo
from tests import trim_model as tm
from tests import util

A1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
A2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
O, E = 5, 10  # the defaults of --adapter-overlap and --adapter-err


def _bytes(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def _upper(c):
    return c & 0xDF if c in b"ACGTacgt" else 0  # a byte that is no letter of ACGTacgt mismatches every letter


def cut(x, A, O=O, E=E):
    """a3 of what the fixed trims leave of a read, x: the bases from the least matching p on, 0 without a match."""
    x, A = _bytes(x), _bytes(A).upper()
    Lp, m = len(x), len(A)
    for p in range(Lp):
        o = min(m, Lp - p)
        mm = sum(1 for j in range(o) if _upper(x[p + j]) != A[j])
        if o >= O and mm * 100 <= o * E:
            return Lp - p
    return 0


def cut_parallel(x, A, O=O, E=E):
    """The same as the kernel does it: per window of 64 positions one occurrence word per letter (bit i: position at + i holds
    the letter; no bit at or past L'), the pair of a window's words and the next one's shifted by the start's lane, ANDed with the
    adapter's occurrence word of the letter and counted; the lowest matching lane of the first window that has one."""
    x, A = _bytes(x), _bytes(A).upper()
    Lp, m = len(x), len(A)
    occ_a = [sum(1 << j for j in range(m) if A[j] == c) for c in b"ACGT"]

    def words(at):
        return [sum(1 << i for i in range(64) if at + i < Lp and _upper(x[at + i]) == c) for c in b"ACGT"]

    cur = words(0)
    for at in range(0, Lp, 64):
        nxt = words(at + 64) if at + 64 < Lp else [0, 0, 0, 0]
        hits = 0
        for ln in range(64):
            matches = sum(bin((((cur[c] | (nxt[c] << 64)) >> ln) & (2 ** 64 - 1)) & occ_a[c]).count("1") for c in range(4))
            o = min(m, Lp - (at + ln))
            if o >= O and (o - matches) * 100 <= o * E:
                hits |= 1 << ln
        if hits:
            return Lp - (at + (hits & -hits).bit_length() - 1)
        cur = nxt
    return 0


def clips(bases, quals, t5, t3, Q, A, O=O, E=E, cut=cut):
    """(c5, c3, a3) of one read: the fixed trims, the adapter match on what they leave (A None: none), the quality rule on the rest."""
    b, q = _bytes(bases), _bytes(quals)
    L = len(b)
    c5 = min(t5, L)
    c3f = min(t3, L - c5)
    a3 = cut(b[c5:L - c3f], A, O, E) if A else 0
    cq = tm.clips(q[c5:L - c3f - a3], 0, 0, Q)[1]
    return c5, c3f + a3 + cq, a3


def cut_np(x, A, O=O, E=E):
    """cut() with the mismatches of all starts counted at once, one adapter letter at a time (for the batches of the tests)."""
    x, A = np.frombuffer(_bytes(x), np.uint8), _bytes(A).upper()
    Lp, m = len(x), len(A)
    if not Lp:
        return 0
    up = np.where(np.isin(x, np.frombuffer(b"ACGTacgt", np.uint8)), x & 0xDF, 0)
    mm = np.zeros(Lp, np.int64)
    for j in range(min(m, Lp)):
        mm[:Lp - j] += up[j:] != A[j]
    o = np.minimum(m, Lp - np.arange(Lp))
    hit = np.flatnonzero((o >= O) & (mm * 100 <= o * E))
    return Lp - int(hit[0]) if len(hit) else 0


def batch_clips(reads, quals, t5, t3, Q, A, O=O, E=E, A2=None, paired=False):
    """[(c5, c3)] and [a3] of a batch; paired: the reads of the second half are matched against A2 (None: A)."""
    half = len(reads) // 2 if paired else len(reads)
    full = [clips(r, q, t5, t3, Q, (A2 or A) if i >= half else A, O, E, cut_np) for i, (r, q) in enumerate(zip(reads, quals))]
    return [(a, b) for a, b, _ in full], [c for _, _, c in full]


def kept(reads, quals, t5, t3, Q, A, O=O, E=E, A2=None, paired=False):
    """-> (the kept parts of the reads, of the qualities, the clips, the adapter cuts)."""
    cl, a3 = batch_clips(reads, quals, t5, t3, Q, A, O, E, A2, paired)
    part = lambda x, c: x[c[0]:len(x) - c[1]]  # noqa: E731
    return [part(r, c) for r, c in zip(reads, cl)], [part(q, c) for q, c in zip(quals, cl)], cl, a3


def counts(a3):
    """(reads with a3 > 0, the sum of a3): the two counters of fem_dev_adapter_count."""
    return sum(1 for a in a3 if a), sum(a3)


# ---- cases ----

def _body(rng, seq, n, e, rev):
    """A reference substring of n bases, reverse-complemented for rev, with 0..e substitutions as trim_model.tailed_reads makes them."""
    at = int(rng.integers(0, len(seq) - n))
    body = bytearray(seq[at:at + n])
    if rev:
        body = bytearray(util.revcomp(bytes(body)))
    for p in rng.choice(len(body), int(rng.integers(0, e + 1)), replace=False):
        body[p] = b"ACGT"[(b"ACGT".index(bytes([body[p]])) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(body)


@functools.lru_cache(maxsize=None)
def readthrough_case():
    """The issue's measured case: seed 5, a random reference of 300 kbp, 600 reads of 120 bases, e = 3; read i has a read-through of
    t = 0..47 bases: the first t bytes of A1 + random, for t >= 33 and i % 4 == 0 with one adapter base substituted."""
    rng = np.random.default_rng(5)
    seqs, names = [util.rand_seq(rng, 300_000)], ["chr0"]
    reads, through = [], []
    for i in range(600):
        t = int(rng.integers(0, 48))
        body = _body(rng, seqs[0], 120 - t, 3, i % 2)
        tail = bytearray((A1 + util.rand_seq(rng, 64))[:t])
        if t >= 33 and i % 4 == 0:
            p = int(rng.integers(0, 33))
            tail[p] = b"ACGT"[(b"ACGT".index(bytes([tail[p]])) + 1 + int(rng.integers(0, 3))) % 4]
        reads.append(body + bytes(tail))
        through.append(t)
    ref = fo.Reference(seqs)
    return dict(seqs=seqs, names=names, reads=reads, quals=["I" * 120] * 600, through=through, rnames=["a%d" % i for i in range(600)], e=3,
                ref=ref, idx=fo.OracleIndex(ref), adapter=A1)


@functools.lru_cache(maxsize=None)
def pairs_case():
    """300 fragments of 73..160 bases, both mates 120 bases: mate 1 = (fragment + A1 + random)[:120], mate 2 = (revcomp(fragment) +
    A2 + random)[:120]; fragments of 120 and more have no adapter.  The reads are mate 1's, then mate 2's."""
    rng = np.random.default_rng(6)
    seqs, names = [util.rand_seq(rng, 300_000)], ["chr0"]
    r1, r2, frag = [], [], []
    for i in range(300):
        f = int(rng.integers(73, 161))
        at = int(rng.integers(0, len(seqs[0]) - f))
        fragment = seqs[0][at:at + f]
        r1.append((fragment + A1 + util.rand_seq(rng, 64))[:120])
        r2.append((util.revcomp(fragment) + A2 + util.rand_seq(rng, 64))[:120])
        frag.append(f)
    ref = fo.Reference(seqs)
    return dict(seqs=seqs, names=names, reads=r1 + r2, quals=["I" * 120] * 600, frag=frag, n=300, rnames=["f%d" % i for i in range(300)], e=2,
                ref=ref, idx=fo.OracleIndex(ref), adapter=A1, adapter2=A2)


ADAPTERS = (4, 31, 32, 33, 63, 64)                    # adapter lengths: a word's half, its whole and one to either side
SETTINGS = ((5, 10), (1, 0), (4, 30), (None, 0))      # (O, E); None: O = m
TRIMS = ((0, 0, 0), (3, 4, 0), (0, 0, 20), (7, 0, 20))


@functools.lru_cache(maxsize=None)
def match_case():
    """One ragged batch of about 2 000 reads -> (A, reads, quals); the adapters of the tests are A[:m] for m in ADAPTERS, so a
    planted A[:m] is a planted A[:m'] for every m' < m as well.  Every length of trim_model.LENGTHS; the adapter planted at
    every residue of p mod 64 in 56..71 and at L - o for o = 2 .. m, whole or cut short by the read's end, with mismatches at the
    thresholds of E = 10 and 30 and one above them, N, = and lower case inside overlaps; reads that are all adapter; reads
    followed in the buffer by a read that begins with the rest of the adapter."""
    rng = np.random.default_rng(100)
    A = util.rand_seq(rng, 64)
    units = []  # lists of reads that stay neighbours

    def plant(L, p, m, mism=0, odd=None):
        r = bytearray(util.rand_seq(rng, L))
        part = bytearray(A[:max(0, min(m, L - p))])
        for j in rng.choice(len(part), min(mism, len(part)), replace=False):
            part[j] = b"ACGT"[(b"ACGT".index(bytes([part[j]])) + 1 + int(rng.integers(0, 3))) % 4]
        if odd and part:
            part[int(rng.integers(0, len(part)))] = odd
        r[p:p + len(part)] = part
        return bytes(r)

    for L in tm.LENGTHS:
        units += [[util.rand_seq(rng, L)], [util.rand_seq(rng, L).lower()]]
        for p in range(0, L, 64):
            for d in range(56, 72):  # starts that straddle the windows' boundaries
                if p + d < L:
                    m = ADAPTERS[int(rng.integers(0, len(ADAPTERS)))]
                    o = min(m, L - p - d)
                    mism = (0, o // 10, o // 10 + 1, 3 * o // 10, 3 * o // 10 + 1)[int(rng.integers(0, 5))]
                    units.append([plant(L, p + d, m, mism)])
        for o in range(2, 65):  # the adapter's first o letters at the read's very end
            if o <= L and (L < 200 or o % 3 == 0 or o < 8 or o > 61):
                k = int(rng.integers(0, 6))
                units.append([(plant(L, L - o, o), plant(L, L - o, o, o // 10), plant(L, L - o, o, o // 10 + 1), plant(L, L - o, o, 0, ord("N")),
                               plant(L, L - o, o, 0, ord("=")), plant(L, L - o, o).lower())[k]])
        if L >= 8:
            for o in (3, 4, 16):  # a read that ends in o letters, directly followed by one that begins with the next ones
                units.append([plant(L, L - o, o), A[o:] + util.rand_seq(rng, 9)])
    for m in ADAPTERS:  # all adapter: p = 0
        units += [[A[:m]], [A[:m].lower()], [A[:m - 1]], [A[:m] + A[:m]]]
    units += [[A * 3], [b""], [plant(65, 60, 64), A[5:] + b"ACGTACGTA"]]
    order = rng.permutation(len(units))
    reads = [r for i in order for r in units[i]]
    quals = [tm.profile_quals(rng, tm.PROFILES[i % len(tm.PROFILES)], len(r), i % 7).decode("latin-1") for i, r in enumerate(reads)]
    return A, reads, quals
