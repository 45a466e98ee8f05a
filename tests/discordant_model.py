"""Plain-Python model of mate rescue with --rescue-discordant (fem_dev_set_rescue_discordant in include/fem_hip.h), on
tests/rescue_model.py, tests/pair_model.py and the oracle's bindings.

A pair is a candidate in two ways.  Kind 1: exactly one mate has no record (tests.rescue_model, unchanged).  Kind 2: both mates
have records and no combination of them is concordant (tests.pair_model.choose).  A kind-2 pair is searched in both directions
(d = 0: mate 2 from mate 1's anchors, d = 1: mate 1 from mate 2's), each anchor by rescue_model's rule; the least
(nm(anchor) + ed, d, anchor index) is traced and kept if start >= 0 and the record is concordant with its anchor.  A kept
kind-2 record goes behind its mate's own records, which all stay; the expected text and arrays are then pair_model's."""
import re

from oracle import fem_oracle as fo
from tests import pair_model as pm
from tests import rescue_model as rm


def _anchors(res, lo, hi):
    """(anchor index, record) of a list's anchors: its first rm.ANCHORS records, those with 0x8000 left out."""
    return [(a, j) for a, j in enumerate(range(lo, min(hi, lo + rm.ANCHORS))) if not int(res.r_flag[j]) & 0x8000]


def rescue_discordant_pair(res, n_pairs, i, reads, seqs, E, I, X, ref=None):
    """A kind-2 pair's rescue: None (no hit in either direction), or rescue_model.rescue_pair's dict with "d" and "tie" added."""
    chosen, sums = None, {}
    for d in (0, 1):
        a_read, b_read = (i, n_pairs + i) if d == 0 else (n_pairs + i, i)
        read = reads[b_read]
        L = len(read)
        for a, j in _anchors(res, int(res.rec_off[a_read]), int(res.rec_off[a_read + 1])):
            fl, tid, pa = int(res.r_flag[j]), int(res.r_tid[j]), int(res.r_pos[j])
            lo, hi, rc = rm.windows(fl, pa, pa + pm.span(res, j), L, I, X)
            if lo > hi:
                continue
            text = fo.revcomp(read) if rc else read
            hit = rm.search(seqs[tid], text, lo, hi, E)
            if hit is None:
                continue
            key = (int(res.r_nm[j]) + hit[0], d, a)
            sums[d] = min(sums.get(d, key[0]), key[0])
            if chosen is None or key < chosen["key"]:
                chosen = dict(key=key, d=d, anchor=j, a=a, hit=hit, rc=rc, tid=tid, text=text, b_read=b_read)
    if chosen is None:
        return None
    chosen["tie"] = len(sums) == 2 and sums[0] == sums[1]  # both directions hit with equal sums (d = 0 is taken)
    ed, pos, c, end = chosen["hit"]
    L = len(chosen["text"])
    text, offs = ref or rm.concatenated(seqs)
    at = offs[chosen["tid"]] + c
    start, cig, md = fo.align(E, text[at:at + L + 4 * E + 64], chosen["text"], ed, end)
    chosen["start"] = start
    chosen["kept"] = False
    if start < 0:
        return chosen
    cigar = [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", cig)]
    rec = (16 if chosen["rc"] else 0, chosen["tid"], c + start, ed, cigar, md)
    chosen["record"] = rec
    j = chosen["anchor"]
    an_f, an_p = int(res.r_flag[j]), int(res.r_pos[j])
    an_e = an_p + pm.span(res, j)
    end0 = rec[2] + sum(n for n, op in cigar if op in "MD")
    if not an_f & 16:  # the anchor forward, the rescued record reverse
        chosen["kept"] = an_p <= rec[2] and I <= end0 - an_p <= X
    else:
        chosen["kept"] = rec[2] <= an_p and I <= an_e - rec[2] <= X
    return chosen


def rescue(res, n_pairs, reads, seqs, E, I=0, X=500):
    """-> (records with the kept rescued records, {read: its rescue} of the kept ones, {pair: rescue} of every traced hit,
    {read: (kind, d)} of the kept ones).  The first three are rescue_model.rescue's on a batch without kind-2 pairs."""
    ref = rm.concatenated(seqs)
    chosen = pm.choose(res, n_pairs, I, X)
    traced, kinds = {}, {}
    for i in range(n_pairs):
        na = int(res.rec_off[i + 1]) - int(res.rec_off[i])
        nb = int(res.rec_off[n_pairs + i + 1]) - int(res.rec_off[n_pairs + i])
        if (na > 0) != (nb > 0):
            r, kind = rm.rescue_pair(res, n_pairs, i, reads, seqs, E, I, X, ref), 1
            d = 0 if na > 0 else 1
        elif na > 0 and chosen[i] is None:
            r, kind = rescue_discordant_pair(res, n_pairs, i, reads, seqs, E, I, X, ref), 2
            d = r["d"] if r is not None else None
        else:
            continue
        if r is not None:
            traced[i] = r
            if r["kept"]:
                kinds[r["b_read"]] = (kind, d)
    kept = {r["b_read"]: r for r in traced.values() if r["kept"]}
    per_read = []
    for rd in range(2 * n_pairs):
        own = [rm._records_of(res, j) for j in range(int(res.rec_off[rd]), int(res.rec_off[rd + 1]))]
        per_read.append(own + [kept[rd]["record"]] if rd in kept else own)
    return pm.Records(per_read), kept, traced, kinds
