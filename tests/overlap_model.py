"""Read-through found from the mates' overlap (fem_dev_set_pair_overlap, FEM map --trim-overlap), the rule in plain
Python.  frag() is the serial rule of include/fem_hip.h, frag_parallel() the same through bit planes and windows of 64 candidates,
the form pair_overlap_kernel has, frag_np() a vectorised form for the batches of the tests; batch_clips() composes the cuts with
the adapter's (tests/adapter_model.py) and with the fixed trims and the quality step of tests/trim_model.py.  The text of a batch
trimmed this way is trim_model.apply of the kept parts' text with these clips."""
import functools

import numpy as np

from tests import adapter_model as am
from tests import trim_model as tm
from tests import util

O, E = 20, 10  # the defaults of --trim-overlap-min and --trim-overlap-err
_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}


def _bytes(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def up(c):
    return c & 0xDF if c in b"ACGTacgt" else 0  # a byte that is no letter of ACGTacgt matches nothing


def frag(x, y, O=O, E=E):
    """F of a pair: x, y what the fixed trims leave of mate 1 and of mate 2.  The largest matching f, 0 without one."""
    x, y = _bytes(x), _bytes(y)
    L1, L2 = len(x), len(y)
    for f in range(max(L1, L2) - 1, 0, -1):
        lo, hi = max(0, f - L2), min(f, L1)
        o = hi - lo
        mm = sum(1 for j in range(lo, hi) if not up(x[j]) or not up(y[f - 1 - j]) or up(x[j]) != _COMP[up(y[f - 1 - j])])
        if o >= O and mm * 100 <= o * E:
            return f
    return 0


def cuts(L1, L2, F):
    """(v3 of mate 1, v3 of mate 2)."""
    return (max(0, L1 - F), max(0, L2 - F)) if F > 0 else (0, 0)


def _planes(s, rc):
    """Three bit planes of s, or of its reverse complement: the two bits of the letter's code (bits 1 and 2 of the upper-case
    byte: A 0, C 1, T 2, G 3; the complement flips the second) and the validity; no bit at or past the length."""
    L = len(s)
    b0 = b1 = ok = 0
    for i in range(L):
        c = up(s[L - 1 - i] if rc else s[i])
        if c:
            code = ((c >> 1) & 3) ^ (2 if rc else 0)
            b0 |= (code & 1) << i
            b1 |= ((code >> 1) & 1) << i
            ok |= 1 << i
    return b0, b1, ok


def frag_parallel(x, y, O=O, E=E):
    """The same as the kernel does it: x and the reverse complement z of y as bit planes; lane ln of a window owns f = top - ln;
    it walks the 64-bit words of the window's union of [lo, hi), takes z's word at bit offset 64 w + L2' - f (of either sign, out
    of two neighbours; nothing outside [0, L2')), and counts the positions valid in both and equal in both code bits; the lowest
    matching lane of the first window that has one."""
    x, y = _bytes(x), _bytes(y)
    L1, L2 = len(x), len(y)
    X, Z = _planes(x, False), _planes(y, True)
    M = 2 ** 64 - 1

    def xword(p, w):
        return (p >> (64 * w)) & M if w >= 0 else 0

    def zbits(p, t):  # bits [t, t + 64) of a plane, t of either sign
        return (p >> t) & M if t >= 0 else (p << -t) & M

    top = max(L1, L2) - 1
    while top >= O:
        f_least = max(top - 63, 1)
        w_lo, w_hi = max(0, f_least - L2) >> 6, (min(top, L1) - 1) >> 6
        hits = 0
        for ln in range(64):
            f = top - ln
            lo, hi = max(0, f - L2), min(f, L1)
            o, s = hi - lo, L2 - f
            matches = 0
            for w in range(w_lo, w_hi + 1):
                t = 64 * w + s
                eq = xword(X[2], w) & zbits(Z[2], t) & ~(xword(X[0], w) ^ zbits(Z[0], t)) & ~(xword(X[1], w) ^ zbits(Z[1], t)) & M
                matches += bin(eq).count("1")
            if f >= 1 and o >= O and (o - matches) * 100 <= o * E:
                hits |= 1 << ln
        if hits:
            return top - ((hits & -hits).bit_length() - 1)
        top -= 64
    return 0


@functools.lru_cache(maxsize=1 << 14)
def _profile(x, y):
    """(f, o, matches) of every candidate f = 1 .. max(L1', L2') - 1 of a pair, the matches of all shifts counted at once, one
    letter at a time; the settings only put thresholds on it."""
    L1, L2 = len(x), len(y)
    f = np.arange(1, max(L1, L2, 1), dtype=np.int64)
    o = np.minimum(f, L1) - np.maximum(0, f - L2)
    if not L1 or not L2 or not len(f):
        return f, o, np.zeros(len(f), np.int64)
    letters = np.frombuffer(b"ACGTacgt", np.uint8)
    ax, ay = np.frombuffer(x, np.uint8), np.frombuffer(y, np.uint8)
    ux = np.where(np.isin(ax, letters), ax & 0xDF, 0)
    uy = np.where(np.isin(ay, letters), ay & 0xDF, 0)[::-1]  # z without the complement: compared with the complement's letter below
    by_shift = np.zeros(L1 + L2 - 1, np.int64)  # index k: the shift s = k - (L1 - 1), the matches sum over j of x[j] == z[j + s]
    for c, cc in _COMP.items():
        by_shift += np.correlate((uy == cc).astype(np.int64), (ux == c).astype(np.int64), "full")
    return f, o, by_shift[(L2 - f) + (L1 - 1)]


def frag_np(x, y, O=O, E=E):
    f, o, matches = _profile(_bytes(x), _bytes(y))
    hit = (o >= O) & ((o - matches) * 100 <= o * E)
    return int(f[hit].max()) if hit.any() else 0


def batch_clips(reads, quals, t5, t3, Q, O=O, E=E, A=None, A2=None, aO=am.O, aE=am.E, frag=frag_np):
    """[(c5, c3)], [v3] and [a3] of a batch of pairs (reads i and n / 2 + i are the mates): the fixed trims, on what they leave the
    overlap's cut and the adapter's (A None: none; the second half against A2, None: A), the larger of the two, and the quality
    rule on the rest."""
    n, half = len(reads), len(reads) // 2
    b = [_bytes(r) for r in reads]
    fixed = [(min(t5, len(r)), min(t3, len(r) - min(t5, len(r)))) for r in b]
    part = [r[c5:len(r) - c3f] for r, (c5, c3f) in zip(b, fixed)]
    v3 = [0] * n
    for i in range(half):
        v3[i], v3[half + i] = cuts(len(part[i]), len(part[half + i]), frag(part[i], part[half + i], O, E))
    a3 = [am.cut_np(p, (A2 or A) if i >= half else A, aO, aE) if A else 0 for i, p in enumerate(part)]
    cl = []
    for r, q, (c5, c3f), v, a in zip(b, quals, fixed, v3, a3):
        cut = max(v, a)
        cl.append((c5, c3f + cut + tm.clips(_bytes(q)[c5:len(r) - c3f - cut], 0, 0, Q)[1]))
    return cl, v3, a3


def kept(reads, quals, t5, t3, Q, O=O, E=E, **kw):
    """-> (the kept parts of the reads, of the qualities, the clips, the overlap cuts, the adapter cuts)."""
    cl, v3, a3 = batch_clips(reads, quals, t5, t3, Q, O, E, **kw)
    part = lambda x, c: x[c[0]:len(x) - c[1]]  # noqa: E731
    return [part(r, c) for r, c in zip(reads, cl)], [part(q, c) for q, c in zip(quals, cl)], cl, v3, a3


def counts(v3):
    """(pairs with F > 0, the sum of v3 over both mates): the two counters of fem_dev_pair_overlap_count.  A matching pair cuts at
    least one base of at least one mate, so the pairs with F > 0 are those with a cut."""
    half = len(v3) // 2
    return sum(1 for i in range(half) if v3[i] + v3[half + i]), sum(v3)


# ---- cases ----

SETTINGS = ((20, 10), (8, 0), (12, 30), (1024, 10))  # (O, E); the last one cuts nothing
TRIMS = am.TRIMS


@functools.lru_cache(maxsize=None)
def random_pairs(n=5000, L=100):
    """n pairs of unrelated random mates of L bases: nothing to cut.  (At O = 8, E = 10 a random pair matches at some f with a
    probability of about 6e-5, the sum of (1 + 3 o [o >= 10]) / 4^o over o = 8 .. 19: 0.3 pairs of 5 000 are expected, and this
    seed's draw has none; at O = 12 and 20 the expectation is below 1e-3.)"""
    rng = np.random.default_rng(22)
    return [util.rand_seq(rng, L) for _ in range(2 * n)]


def _subst(rng, c):
    return b"ACGT"[(b"ACGT".index(bytes([c]).upper()) + 1 + int(rng.integers(0, 3))) % 4]


@functools.lru_cache(maxsize=None)
def match_case():
    """One ragged batch of about 1 500 pairs -> (reads, quals), mates 1 then mates 2.  A pair of a fragment of f bases is mate 1 =
    (fragment + random)[:L1], mate 2 = (revcomp(fragment) + random)[:L2].  Every mate length of trim_model.LENGTHS with every
    other; fragments at every residue of max(L) - 1 - f mod 64 in 56..71; shifts L2 - f of 0, +-1, 63, 64, 65; f between min(L)
    and max(L); f = max(L) - 1 and f, o = O - 1, O, O + 1; mismatches at the thresholds of E = 10 and 30 and one above; N, = and
    lower case inside overlaps, an N in both mates at aligned places; tandem repeats; pairs followed in the buffer by reads that
    would complete their match; unrelated and empty mates."""
    rng = np.random.default_rng(200)
    units = []  # lists of pairs (mate 1, mate 2) that stay neighbours in both halves of the buffer

    def pair(L1, L2, f, mism=0, odd=None, unit=0):
        fragment = (util.rand_seq(rng, unit) * (f // unit + 1))[:f] if unit else util.rand_seq(rng, f)
        m1 = bytearray((fragment + util.rand_seq(rng, L1))[:L1])
        m2 = bytearray((util.revcomp(fragment) + util.rand_seq(rng, L2))[:L2])
        lo, hi = max(0, f - L2), min(f, L1)
        if hi > lo:
            for j in rng.choice(hi - lo, min(mism, hi - lo), replace=False):
                m1[lo + j] = _subst(rng, m1[lo + j])
            j = lo + int(rng.integers(0, hi - lo))
            if odd == "N":
                m1[j] = ord("N")
            elif odd == "=":
                m2[f - 1 - j] = ord("=")
            elif odd == "NN":
                m1[j] = m2[f - 1 - j] = ord("N")
            elif odd == "lower":
                m1, m2 = bytearray(bytes(m1).lower()), bytearray(bytes(m2[:L2 // 2]) + bytes(m2[L2 // 2:]).lower())
        return bytes(m1), bytes(m2)

    def steps(o):
        return (0, o // 10, o // 10 + 1, 3 * o // 10, 3 * o // 10 + 1)

    def overlap(L1, L2, f):
        return min(f, L1) - max(0, f - L2)

    for L1 in tm.LENGTHS:  # every length with every other, the mates drawn independently
        for L2 in tm.LENGTHS:
            top, low = max(L1, L2), min(L1, L2)
            if top < 2:
                units.append([(util.rand_seq(rng, L1), util.rand_seq(rng, L2))])
                continue
            for f in (int(rng.integers(max(1, low // 2), top)), int(rng.integers(min(low, top - 1), top)), int(rng.integers(1, top))):
                o = overlap(L1, L2, f)
                units.append([pair(L1, L2, f, steps(o)[int(rng.integers(0, 5))])])
    for top in (100, 129, 193, 1024):  # candidates on either side of the windows' edges
        for k, d in enumerate(list(range(56, 72)) + list(range(120, 136))):
            other = [L for L in tm.LENGTHS if L <= top][int(rng.integers(0, sum(1 for L in tm.LENGTHS if L <= top)))]
            L1, L2 = (top, other) if k % 2 else (other, top)
            f = top - 1 - d
            if f >= 1:
                units.append([pair(L1, L2, f, steps(overlap(L1, L2, f))[k % 5])])
    for d in range(64):  # ... and every lane of the second window
        units.append([pair(150, 150, 149 - 64 - d)])
    for L2 in (64, 65, 100, 128, 129, 193):  # the shift of z against x
        for L1 in (100, 129, 200):
            for s in (0, 1, -1, 63, 64, 65):
                f = L2 - s
                if 1 <= f < max(L1, L2):
                    units.append([pair(L1, L2, f)])
    for L1, L2 in ((36, 36), (100, 64), (64, 100), (129, 129), (1024, 1024)):  # the first candidate, and those around O
        for f in (max(L1, L2) - 1, 7, 8, 9, 11, 12, 13, 19, 20, 21):
            units.append([pair(L1, L2, f)])
    for short in (7, 8, 9, 11, 12, 13, 19, 20, 21):  # ... and overlaps around O on a long fragment
        units += [[pair(100, short, 50)], [pair(short, 100, 50)], [pair(100, 60 + short, 60)]]
    for L1, L2 in ((100, 100), (129, 64), (64, 129), (150, 150)):  # mismatches at the thresholds and one above
        for f in (40, 55, 63):
            for mism in steps(overlap(L1, L2, f)):
                units.append([pair(L1, L2, f, mism)])
    for odd in ("N", "=", "NN", "lower"):
        for L1, L2, f in ((100, 100, 60), (129, 100, 110), (64, 193, 30), (150, 150, 149), (36, 35, 25)):
            units += [[pair(L1, L2, f, 0, odd)], [pair(L1, L2, f, overlap(L1, L2, f) // 10, odd)]]
    for unit in (1, 2, 3, 5, 7, 13):  # tandem repeats: several f match, the largest is the one
        for L1, L2, f in ((100, 100, 60), (129, 100, 110), (100, 129, 90), (150, 150, 149), (193, 193, 70)):
            units.append([pair(L1, L2, f, 0, None, unit)])
    for L_short, f in ((12, 30), (15, 40), (19, 64), (5, 25)):  # the next read in the buffer holds what a short mate lacks
        fragment = util.rand_seq(rng, f)
        rest = util.rand_seq(rng, 40)
        units.append([(fragment[:L_short], (util.revcomp(fragment) + rest)[:f + 10]), (fragment[L_short:] + rest[:9], util.rand_seq(rng, 30))])
        units.append([((fragment + rest)[:f + 10], util.revcomp(fragment)[:L_short]), (util.rand_seq(rng, 30), util.revcomp(fragment)[L_short:] + rest[:9])])
    for L in tm.LENGTHS:  # unrelated mates
        units.append([(util.rand_seq(rng, L), util.rand_seq(rng, L))])
    order = rng.permutation(len(units))
    pairs = [p for i in order for p in units[i]]
    reads = [a for a, _ in pairs] + [b for _, b in pairs]
    quals = [tm.profile_quals(rng, tm.PROFILES[i % len(tm.PROFILES)], len(r), i % 7).decode("latin-1") for i, r in enumerate(reads)]
    return reads, quals
