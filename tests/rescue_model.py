"""Plain-Python model of mate rescue (FEM map --rescue; fem_dev_set_rescue in include/fem_hip.h), on the oracle's bindings.

Input: the single-end records of a batch of 2 n reads (pair i = read i and read n + i) as fo.map_reads returns them, the reads,
the reference sequences, E and the insert range.  Output: the records with every kept rescued mate as its read's only record
(a tests.pair_model.Records), and the kept rescues.  The expected paired text and arrays are then tests.pair_model's on them."""
import re

from oracle import fem_oracle as fo
from tests import pair_model as pm

ANCHORS = 8


def _records_of(res, j):
    ops = res.cig[int(res.cig_off[j]):int(res.cig_off[j + 1])]
    return (int(res.r_flag[j]), int(res.r_tid[j]), int(res.r_pos[j]), int(res.r_nm[j]),
            [(int(o) >> 4, "MID"[int(o) & 0xF]) for o in ops], res.md_str(j))


def _span(cigar):
    return sum(n for n, op in cigar if op in "MD")


def windows(flag, pa, ea, L, I, X):
    """(lo, hi, searched reverse-complemented) of B's pos0 for an anchor."""
    if not flag & 16:
        return max(pa, pa + I - L), pa + X - L, True
    return max(0, ea - X), min(pa, ea - I), False


def search(seq, text, lo, hi, E):
    """The anchor's best hit (ed, pos0, c, end) over its tiles, or None."""
    L, W = len(text), 2 * E + 1
    best = None
    for c in range(lo, hi + 1, W):
        if c + L + 2 * E > len(seq):
            continue
        ed, end = fo.banded_ed32(E, seq[c:c + L + 2 * E], text)
        if ed > E:
            continue
        pos = c + end - L + 1
        if pos <= hi and (best is None or (ed, pos) < best[:2]):
            best = (ed, pos, c, end)
    return best


def concatenated(seqs):
    """The reference as one text (the sequences back to back, 64 zero bytes behind: fo.Reference's and the device's layout)
    and each sequence's offset in it."""
    offs, at = [], 0
    for s in seqs:
        offs.append(at)
        at += len(s)
    return b"".join(seqs) + b"\0" * 64, offs


def rescue_pair(res, n_pairs, i, reads, seqs, E, I, X, ref=None):
    """Pair i's rescue: None (not a candidate, no hit), or a dict with the chosen hit, its record and whether it is kept.
    ref: concatenated(seqs), if made already."""
    a0, a1 = int(res.rec_off[i]), int(res.rec_off[i + 1])
    b0, b1 = int(res.rec_off[n_pairs + i]), int(res.rec_off[n_pairs + i + 1])
    if (a1 > a0) == (b1 > b0):
        return None
    A, b_read = (range(a0, a1), n_pairs + i) if a1 > a0 else (range(b0, b1), i)
    read = reads[b_read]
    L = len(read)
    if L == 0:  # a mate without a base is never searched: it stays unmapped
        return None
    chosen = None
    for a, j in enumerate(list(A)[:ANCHORS]):
        fl = int(res.r_flag[j])
        if fl & 0x8000:
            continue
        tid, pa = int(res.r_tid[j]), int(res.r_pos[j])
        ea = pa + pm.span(res, j)
        lo, hi, rc = windows(fl, pa, ea, L, I, X)
        if lo > hi:
            continue
        text = fo.revcomp(read) if rc else read
        hit = search(seqs[tid], text, lo, hi, E)
        if hit is not None and (chosen is None or (int(res.r_nm[j]) + hit[0], a) < chosen["key"]):
            chosen = dict(key=(int(res.r_nm[j]) + hit[0], a), anchor=j, a=a, hit=hit, rc=rc, tid=tid, text=text, b_read=b_read)
    if chosen is None:
        return None
    ed, pos, c, end = chosen["hit"]
    # the traceback reads the reference itself, the concatenation (beyond the window where the 'S' fold leaves it: into the
    # next sequence, or the zeros behind the last); it reads < L + 4E bases from the window's start
    text, offs = ref or concatenated(seqs)
    at = offs[chosen["tid"]] + c
    start, cig, md = fo.align(E, text[at:at + L + 4 * E + 64], chosen["text"], ed, end)
    chosen["start"] = start
    chosen["kept"] = False
    if start < 0:
        return chosen
    cigar = [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", cig)]
    rec = (16 if chosen["rc"] else 0, chosen["tid"], c + start, ed, cigar, md)
    chosen["record"] = rec
    # concordant with its anchor (the pairing rule, the real CIGAR span)
    j = chosen["anchor"]
    an_f, an_p = int(res.r_flag[j]), int(res.r_pos[j])
    an_e = an_p + pm.span(res, j)
    fwd, rev = ((an_p, an_e), (rec[2], rec[2] + _span(cigar))) if not an_f & 16 else ((rec[2], None), (an_p, an_e))
    ins = rev[1] - fwd[0]
    chosen["kept"] = fwd[0] <= rev[0] and I <= ins <= X
    return chosen


def rescue(res, n_pairs, reads, seqs, E, I=0, X=500):
    """-> (records with the kept rescued mates, {read: its rescue} of the kept ones, {pair: rescue} of every traced hit)."""
    traced = {}
    ref = concatenated(seqs)
    for i in range(n_pairs):
        r = rescue_pair(res, n_pairs, i, reads, seqs, E, I, X, ref)
        if r is not None:
            traced[i] = r
    kept = {r["b_read"]: r for r in traced.values() if r["kept"]}
    per_read = []
    for rd in range(2 * n_pairs):
        if rd in kept:
            per_read.append([kept[rd]["record"]])
        else:
            per_read.append([_records_of(res, j) for j in range(int(res.rec_off[rd]), int(res.rec_off[rd + 1]))])
    return pm.Records(per_read), kept, traced
