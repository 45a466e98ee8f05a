"""Plain-Python model of the mapping qualities of FEM map --mapq (fem_dev_set_mapq in include/fem_hip.h).

The rule.  Q(g, c) = min(60, max(0, 20 g - 3 floor(log2 c))) for a gap of g >= 1 edits and c >= 1 alternatives: 20 per edit
of gap (each extra edit in a short read makes a hit about 100 times less likely), 3 per doubling of the alternatives
(10 log10 2), a cap of 60 as bwa-mem and minimap2 use.  Integers only: floor(log2 c) = 31 - clz(c).

Single-end value of a read r mapped at -e e, from its records as single-end mapping makes them (NM non-decreasing; every
record counts, 0x8000 included; none merged by locus): d1 = NM of the first record, c1 = records with NM = d1.  c1 >= 2:
q_se(r) = 0.  Else d2 = the least NM above d1 and c2 = records with NM = d2 (none: d2 = e + 1, c2 = 1), q_se(r) = Q(d2 - d1, c2).
Single-end lines: a read's primary line gets q_se(r), every other line 0.

Pair mode (a rescued record is its mate's only record).  Not a proper pair: each mate's primary line gets q_se(mate), every
other line 0.  Proper pair with chosen combination (a, b): s1 = nm(a) + nm(b), cp1 = concordant combinations with sum s1,
s2 = the least concordant sum above s1, cp2 = how many have it; qp = 0 if cp1 >= 2, 60 if there is no s2, else
Q(s2 - s1, cp2).  For the chosen record x of a mate, q_x = q_se(mate) if x is not rescued and nm(x) = d1(mate), else 0; the
mate's primary line gets max(q_x, min(qp, q_x + 40)), every other line (0x100) 0.  "Concordant" is tests.pair_model's rule.

Input: the oracle's single-end records (fo.map_reads), tests.pair_model.choose for pairs, tests.rescue_model.rescue for
rescued lists.  from_sam() recomputes the qualities from the SAM text of a run without --mapq (single-end, or paired without
rescue): the text shows everything the rule reads except 0x8000, so it is for generated ACGT data only, where no record
carries it."""
import re

import numpy as np

from tests import pair_model as pm


def Q(g, c):
    return min(60, max(0, 20 * g - 3 * (int(c).bit_length() - 1)))


def q_se(nms, e):
    """The single-end value of a read whose records have these NM values, in single-end order (none: 0, it has no line)."""
    nms = [int(x) for x in nms]
    if not nms:
        return 0
    d1 = nms[0]
    if sum(1 for x in nms if x == d1) >= 2:
        return 0
    above = [x for x in nms if x > d1]
    d2 = min(above) if above else e + 1
    c2 = sum(1 for x in above if x == d2) if above else 1
    return Q(d2 - d1, c2)


def _read_nms(res, r):
    return res.r_nm[int(res.rec_off[r]):int(res.rec_off[r + 1])]


def single_end(res, e):
    """Per line (record order), the MAPQ of the single-end text."""
    out = []
    for r in range(len(res.rec_off) - 1):
        n = int(res.rec_off[r + 1]) - int(res.rec_off[r])
        if n:
            out += [q_se(_read_nms(res, r), e)] + [0] * (n - 1)
    return out


def combine(q_x, qp):
    return max(q_x, min(qp, q_x + 40))


def pair_qp(sums, s1):
    """qp of a proper pair from its concordant sums (numpy array) and the chosen sum s1."""
    if int(np.count_nonzero(sums == s1)) >= 2:
        return 0
    above = sums[sums > s1]
    if not len(above):
        return 60
    s2 = int(above.min())
    return Q(s2 - s1, int(np.count_nonzero(above == s2)))


def _concordant_sums(fa, ta, pa, ea, na, fb, tb, pb, eb, nb, I, X):
    """The sums of every concordant combination of lists A and B (numpy arrays of flag, tid, pos0, end0, nm)."""
    out = []
    okb = (fb & 0x8000) == 0
    for k in range(len(fa)):
        if int(fa[k]) & 0x8000:
            continue
        ok = okb & (tb == int(ta[k])) & (((fb ^ int(fa[k])) & 16) != 0)
        if int(fa[k]) & 16:  # a reverse, b forward
            ins = int(ea[k]) - pb
            ok &= pb <= int(pa[k])
        else:
            ins = eb - int(pa[k])
            ok &= int(pa[k]) <= pb
        ok &= (ins >= I) & (ins <= X)
        out.append(nb[ok] + int(na[k]))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def _lists(res, lo, hi):
    j = np.arange(lo, hi)
    f = res.r_flag[lo:hi].astype(np.int64)
    t = res.r_tid[lo:hi].astype(np.int64)
    p = res.r_pos[lo:hi].astype(np.int64)
    e = p + np.array([pm.span(res, x) for x in j], np.int64)
    return f, t, p, e, res.r_nm[lo:hi].astype(np.int64)


def paired(se, n_pairs, e, I=0, X=500, res=None, rescued=()):
    """Per line, in tests.pair_model.expected's order, the MAPQ of the paired text.  se: the single-end records (q_se, d1);
    res: the lists pairing sees (rescue_model.rescue's records; default se); rescued: the reads whose list is a rescued record."""
    res = se if res is None else res
    chosen = pm.choose(res, n_pairs, I, X)
    order = pm.line_order(res, n_pairs, chosen)
    out = []
    for i in range(n_pairs):
        reads = (i, n_pairs + i)
        qs = [q_se(_read_nms(se, r), e) for r in reads]
        c = chosen[i]
        if c is None:
            prim = qs
        else:
            A = _lists(res, int(res.rec_off[i]), int(res.rec_off[i + 1]))
            B = _lists(res, int(res.rec_off[n_pairs + i]), int(res.rec_off[n_pairs + i + 1]))
            s1 = int(A[4][c[0]]) + int(B[4][c[1]])
            qp = pair_qp(_concordant_sums(*A, *B, I, X), s1)
            prim = []
            for m, r in enumerate(reads):
                x = int(res.rec_off[r]) + c[m]
                own = r not in rescued and len(_read_nms(se, r)) and int(res.r_nm[x]) == int(_read_nms(se, r)[0])
                prim.append(combine(qs[m] if own else 0, qp))
        for m in (0, 1):
            n = len(order[2 * i + m])
            if n:
                out += [prim[m]] + [0] * (n - 1)
    return out


def with_mapq(text, mapqs):
    """SAM lines (bytes or str, no header) with column 5 replaced, line by line."""
    as_bytes = isinstance(text, bytes)
    lines = (text.decode("latin-1") if as_bytes else text).splitlines()
    assert len(lines) == len(mapqs)
    out = "".join("\t".join(f[:4] + [str(q)] + f[5:]) + "\n" for f, q in ((l.split("\t"), q) for l, q in zip(lines, mapqs)))
    return out.encode("latin-1") if as_bytes else out


def column5(text):
    t = text.decode("latin-1") if isinstance(text, bytes) else text
    return [int(l.split("\t")[4]) for l in t.splitlines() if l and not l.startswith("@")]


def _span_of(cigar):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MDN=X")


def from_sam(text, e, paired_mode=False, I=0, X=500):
    """Per line (header lines skipped), the MAPQ the rule gives the lines of a text made without --mapq (ACGT data only)."""
    t = text.decode("latin-1") if isinstance(text, bytes) else text
    rows = [l.split("\t") for l in t.splitlines() if l and not l.startswith("@")]
    groups = []  # one per read (mate): its lines, primary first
    for k, f in enumerate(rows):
        if not int(f[1]) & 256:
            groups.append([])
        groups[-1].append(k)
    nm = [int(next(x for x in f[11:] if x.startswith("NM:i:"))[5:]) for f in rows]
    out = [0] * len(rows)
    if not paired_mode:
        for g in groups:
            out[g[0]] = q_se([nm[k] for k in g], e)
        return out

    def q_mate(g):  # single-end order is NM order: the least NM is d1
        return q_se(sorted(nm[k] for k in g), e)

    def arrays(g):
        fl = np.array([int(rows[k][1]) for k in g], np.int64)
        tid = np.array([hash(rows[k][2]) for k in g], np.int64)
        pos = np.array([int(rows[k][3]) - 1 for k in g], np.int64)
        end = pos + np.array([_span_of(rows[k][5]) for k in g], np.int64)
        return fl, tid, pos, end, np.array([nm[k] for k in g], np.int64)

    k = 0
    while k < len(groups):
        g = groups[k]
        f0 = rows[g[0]]
        mates = [g]
        if int(f0[1]) & 0x40 and k + 1 < len(groups) and rows[groups[k + 1][0]][0] == f0[0] and int(rows[groups[k + 1][0]][1]) & 0x80:
            mates.append(groups[k + 1])
        k += len(mates)
        if not int(f0[1]) & 2:
            for m in mates:
                out[m[0]] = q_mate(m)
            continue
        a, b = mates
        s1 = nm[a[0]] + nm[b[0]]
        qp = pair_qp(_concordant_sums(*arrays(a), *arrays(b), I, X), s1)
        for m in mates:
            own = nm[m[0]] == min(nm[j] for j in m)
            out[m[0]] = combine(q_mate(m) if own else 0, qp)
    return out
