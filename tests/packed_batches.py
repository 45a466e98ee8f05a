"""Batches for the tests of the packed read forms (test_gpu_select_packed): a small reference with planted repeats and
near-copies, reads with edits on both strands, and reads carrying characters the packed form sends separately."""
import numpy as np

from tests import util

UNIT, UNIT_COPIES = 300, 12
LONG_UNIT = 1500


def clustered(rng, s, cluster, period):
    """A near-copy: `cluster` consecutive substitutions every `period` bases — a read over it is beyond e edits where a
    cluster of e + 2 falls inside it, and still shares whole seeds with the original between the clusters."""
    s = bytearray(s)
    for at in range(int(rng.integers(3, period)), len(s) - cluster, period):
        for i in range(at, at + cluster):
            s[i] = util.ACGT[(np.searchsorted(util.ACGT, s[i]) + 1 + rng.integers(0, 3)) % 4]
    return bytes(s)


def reference(rng):
    """Four sequences of 20-60 kbp: a 300-base unit in 12 copies, three near-copies of it, a 1500-base unit twice with three
    near-copies (decoys for reads longer than the short unit), a 60-base repeat five times."""
    unit, long_unit, short = util.rand_seq(rng, UNIT), util.rand_seq(rng, LONG_UNIT), util.rand_seq(rng, 60)
    near = [(2, 14), (5, 30), (9, 45)]  # clusters of e + 2 for e = 0, 3, 7 (e = 1: two clusters of the first)
    pieces = [unit] * UNIT_COPIES + [clustered(rng, unit, c, p) for c, p in near]
    pieces += [long_unit] * 2 + [clustered(rng, long_unit, c, p) for c, p in near] + [short] * 5
    order = rng.permutation(len(pieces))
    seqs, places = [], []  # places: (sequence, offset, length) of the exact copies of the two units
    lens = [20_000, 35_000, 45_000, 60_000]
    per_seq = [[] for _ in lens]
    for j, pi in enumerate(order):
        per_seq[j % len(lens)].append(int(pi))
    for si, total in enumerate(lens):
        parts, used = [], 0
        gap = (total - sum(len(pieces[pi]) for pi in per_seq[si])) // (len(per_seq[si]) + 1)
        for pi in per_seq[si]:
            parts.append(util.rand_seq(rng, gap))
            used += gap
            if pi < UNIT_COPIES or len(pieces) - 5 - 3 - 2 <= pi < len(pieces) - 5 - 3:
                places.append((si, used, len(pieces[pi])))
            parts.append(pieces[pi])
            used += len(pieces[pi])
        parts.append(util.rand_seq(rng, total - used))
        seqs.append(b"".join(parts))
    return seqs, places


def edit(rng, s, n_err, L):
    """n_err edits (substitutions, insertions, deletions) anywhere — the first and last three bases included."""
    s = bytearray(s)
    for _ in range(n_err):
        u = rng.random()
        pos = int(rng.integers(0, 3)) if u < 0.2 else L - 1 - int(rng.integers(0, 3)) if u < 0.4 else int(rng.integers(0, L))
        r = rng.random()
        if r < 0.6:
            s[pos] = util.ACGT[(np.searchsorted(util.ACGT, s[pos]) + 1 + rng.integers(0, 3)) % 4]
        elif r < 0.8:
            s.insert(pos, int(util.ACGT[rng.integers(0, 4)]))
        else:
            del s[pos]
    return bytes(s[:L])


def reads(rng, seqs, places, n, L, e):
    """Half of the reads from inside the planted units (many candidates, decoys among them), half from anywhere; both
    strands; 0..e edits.  Reads 0 and n - 1 are exact and on the reverse strand: they load at the packed buffer's edges."""
    fit = [p for p in places if p[2] >= L + e]
    out = []
    for i in range(n):
        if fit and rng.random() < 0.5:
            si, at, ln = fit[int(rng.integers(0, len(fit)))]
            start = at + int(rng.integers(0, ln - (L + e) + 1))
        else:
            si = int(rng.integers(0, len(seqs)))
            start = int(rng.integers(0, len(seqs[si]) - (L + e) - 1))
        w = seqs[si][start:start + L + e]
        edge = i == 0 or i == n - 1
        r = w[:L] if edge else edit(rng, w, int(rng.integers(0, e + 1)), L)
        out.append(util.revcomp(r) if edge or rng.random() < 0.5 else r)
    return out


def exceptions(rng, reads, share):
    """A share of the reads carries one to three of N, n, a lower-case base and R, at the first, a middle and the last base.
    Returns the reads and, per read, 0 (untouched), 1 (lower-case bases only: same outcome as in upper case) or 2."""
    out, kind = [], np.zeros(len(reads), np.int8)
    for i, r in enumerate(reads):
        if rng.random() < share:
            r = bytearray(r)
            L = len(r)
            lower_only = rng.random() < 0.4
            places = [0, L // 2, L - 1]
            for at in [places[int(j)] for j in rng.permutation(3)[:int(rng.integers(1, 4))]]:
                r[at] = r[at] | 0x20 if lower_only else int(rng.choice([ord("N"), ord("n"), r[at] | 0x20, ord("R")]))
            kind[i] = 1 if lower_only else 2
            r = bytes(r)
        out.append(r)
    return out, kind
