"""Plain-Python model of the library orientations (FEM map --orientation; fem_dev_set_orientation and fem_dev_estimate_library
in include/fem_hip.h).  The rule stands here twice.

1. Directly: insert_of, choose and expected below, written out from the table of flips: the virtual strand of a record of mate m
   is its strand XOR flip_m, and the pairing rule reads virtual strands.
2. By reduction to the FR models: virtual() is a shallow copy of the records with 16 flipped on the records of flipped mates,
   virtual_reads() the reads with those of flipped mates reverse-complemented.  These go unchanged to pair_model, rescue_model,
   discordant_model, mapq_model, unmapped_model and insert_model; real_flag / real_lines / real_text / real_arrays / real_records
   map what they return back: 0x10 ^= flip(own mate) on a mapped line, 0x20 ^= flip(other mate) where the other mate has a
   record, a rescued record's 16 ^= flip(its mate); TLEN and everything else as returned.  SEQ is the read as staged, so the
   text models are given the staged reads, the searching models the virtual ones.

Reads that go through a rescue model hold upper-case A C G T N only, so that reverse-complementing twice is the identity.
library_estimate is the model of fem_dev_estimate_library, its choice and ties included."""
import copy

import numpy as np

from tests import discordant_model as dm
from tests import insert_model as im
from tests import pair_model as pm
from tests import rescue_model as rm
from tests import unmapped_model as um

FR, RF, FF = 0, 1, 2
NAMES = ("fr", "rf", "ff")
FLIPS = {FR: (0, 0), RF: (1, 1), FF: (0, 1)}  # (flip1, flip2)

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    """Reverse complement of upper-case A C G T N (N stays N)."""
    assert not set(s) - set(b"ACGTN"), "reads of an orientation test are upper-case A C G T N"
    return s.translate(_COMP)[::-1]


# ---- 1. the rule, directly ----

def insert_of(res, ja, jb, min_insert, max_insert, orient):
    """The insert of record ja of mate 1 and record jb of mate 2 if the combination is concordant, else None."""
    f1, f2 = FLIPS[orient]
    fa, fb = int(res.r_flag[ja]), int(res.r_flag[jb])
    if (fa | fb) & 0x8000 or int(res.r_tid[ja]) != int(res.r_tid[jb]):
        return None
    va, vb = bool(fa & 16) ^ bool(f1), bool(fb & 16) ^ bool(f2)  # virtual strands: True = reverse
    if va == vb:
        return None
    f, r = (jb, ja) if va else (ja, jb)
    if int(res.r_pos[f]) > int(res.r_pos[r]):
        return None
    ins = int(res.r_pos[r]) + pm.span(res, r) - int(res.r_pos[f])
    return ins if min_insert <= ins <= max_insert else None


def choose(res, n_pairs, min_insert, max_insert, orient):
    """Per pair: (index a, index b, insert) of the chosen combination (least NM sum, then a, then b), or None."""
    out = []
    for i in range(n_pairs):
        a0, a1 = int(res.rec_off[i]), int(res.rec_off[i + 1])
        b0, b1 = int(res.rec_off[n_pairs + i]), int(res.rec_off[n_pairs + i + 1])
        best = None
        for ja in range(a0, a1):
            for jb in range(b0, b1):
                ins = insert_of(res, ja, jb, min_insert, max_insert, orient)
                if ins is None:
                    continue
                key = (int(res.r_nm[ja]) + int(res.r_nm[jb]), ja - a0, jb - b0)
                if best is None or key < best[0]:
                    best = (key, ins)
        out.append(None if best is None else (best[0][1], best[0][2], best[1]))
    return out


def expected(res, n_pairs, min_insert, max_insert, orient):
    """pair_model.expected's lines and proper-pair count under `orient`, from the rule directly: FLAG 0x10 and 0x20 the real
    strands, TLEN +ins on the virtually forward mate's primary line."""
    chosen = choose(res, n_pairs, min_insert, max_insert, orient)
    order = pm.line_order(res, n_pairs, chosen)
    lines = []
    for i in range(n_pairs):
        c = chosen[i]
        for m in (0, 1):
            recs, other = order[2 * i + m], order[2 * i + 1 - m]
            o = other[0] if other else None
            for t, j in enumerate(recs):
                fl = int(res.r_flag[j])
                flag = (fl & 0x8010) | 0x1 | (0x80 if m else 0x40) | (256 if t else 0)
                tlen = 0
                if c is not None and t == 0:
                    flag |= 0x2
                    tlen = -c[2] if bool(fl & 16) ^ bool(FLIPS[orient][m]) else c[2]
                if o is None:
                    flag |= 0x8
                elif int(res.r_flag[o]) & 16:
                    flag |= 0x20
                lines.append((i if m == 0 else n_pairs + i, j, flag, None if o is None else int(res.r_tid[o]),
                              None if o is None else int(res.r_pos[o]), tlen))
    return lines, sum(x is not None for x in chosen)


# ---- 2. the reduction to the FR models ----

def _flipped_records(res, n_pairs, orient):
    """Boolean per record: it belongs to a flipped mate."""
    f1, f2 = FLIPS[orient]
    mid, end = int(res.rec_off[n_pairs]), int(res.rec_off[2 * n_pairs])
    m = np.zeros(len(res.r_flag), bool)
    m[:mid], m[mid:end] = bool(f1), bool(f2)
    return m


def virtual(res, n_pairs, orient):
    """The records as the FR models are to see them: a shallow copy, 16 flipped on the records of flipped mates.  It is its own
    inverse (real_records)."""
    v = copy.copy(res)
    v.r_flag = np.where(_flipped_records(res, n_pairs, orient), res.r_flag ^ np.uint16(16), res.r_flag).astype(res.r_flag.dtype)
    return v


real_records = virtual


def virtual_reads(reads, n_pairs, orient):
    f1, f2 = FLIPS[orient]
    return [revcomp(r) if (f2 if k >= n_pairs else f1) else r for k, r in enumerate(reads)]


def real_flag(flag, orient):
    """A line's FLAG back from the virtual world."""
    f1, f2 = FLIPS[orient]
    own, other = (f2, f1) if flag & 0x80 else (f1, f2)
    if own and not flag & 0x4:
        flag ^= 0x10
    if other and not flag & 0x8:
        flag ^= 0x20
    return flag


def real_lines(lines, orient):
    """pair_model.expected's line tuples back from the virtual world."""
    return [(r, j, real_flag(flag, orient), mt, mp, tlen) for r, j, flag, mt, mp, tlen in lines]


def real_text(text, orient):
    """A paired SAM text (bytes or str, no header) back from the virtual world: column 2."""
    as_bytes = isinstance(text, bytes)
    out = []
    for l in (text.decode("latin-1") if as_bytes else text).splitlines():
        f = l.split("\t")
        f[1] = str(real_flag(int(f[1]), orient))
        out.append("\t".join(f) + "\n")
    return "".join(out).encode("latin-1") if as_bytes else "".join(out)


def real_arrays(arrays, orient):
    """pair_model.pair_arrays' dict back from the virtual world (the flag column; 0x8000 kept)."""
    out = dict(arrays)
    out["flag"] = np.array([real_flag(int(f), orient) for f in arrays["flag"]], np.uint16)
    return out


def rescued(res, n_pairs, reads, seqs, E, I, X, orient, discordant=False):
    """The rescue models on the virtual batch -> (virtual records with the kept rescued ones, {read: kept rescue}, {pair: traced
    rescue}, {read: (kind, d)}); each rescue dict gets "real_flag", its record's FLAG 16 in the real world."""
    v, vr = virtual(res, n_pairs, orient), virtual_reads(reads, n_pairs, orient)
    if discordant:
        ext, kept, traced, kinds = dm.rescue(v, n_pairs, vr, seqs, E, I, X)
    else:
        ext, kept, traced = rm.rescue(v, n_pairs, vr, seqs, E, I, X)
        kinds = {r: (1, 0 if r >= n_pairs else 1) for r in kept}
    for r in traced.values():
        flip_b = FLIPS[orient][1 if r["b_read"] >= n_pairs else 0]
        r["real_flag"] = (16 if r["rc"] else 0) ^ (16 if flip_b else 0)
    return ext, kept, traced, kinds


def paired_text(res, n_pairs, seq_names, reads, names, quals, I, X, orient, ext=None, rescued_reads=(), e=None, unmapped=False):
    """The paired text (bytes) under `orient` through unmapped_model.paired (MAPQ with e, the unmapped reads' lines with
    `unmapped`).  ext: rescued()'s virtual records."""
    v = virtual(res, n_pairs, orient)
    text = um.paired(v, n_pairs, seq_names, reads, names, quals, I, X, res=ext, rescued=rescued_reads, e=e)
    if not unmapped:
        text = um.without_unmapped(text, True)[0]
    return real_text(text, orient)


def pair_arrays(res, n_pairs, I, X, orient, ext=None):
    """The fem_batch_pairs arrays under `orient` (ext: rescued()'s virtual records)."""
    return real_arrays(pm.pair_arrays(virtual(res, n_pairs, orient) if ext is None else ext, n_pairs, I, X), orient)


# ---- the library estimate ----

def estimate(res, n_pairs, orient):
    """fem_dev_estimate_insert with `orient` set, from the rule directly (insert_model's fields)."""
    n_unique, ins = 0, []
    for i in range(n_pairs):
        a0, a1 = int(res.rec_off[i]), int(res.rec_off[i + 1])
        b0, b1 = int(res.rec_off[n_pairs + i]), int(res.rec_off[n_pairs + i + 1])
        if a1 - a0 != 1 or b1 - b0 != 1 or (int(res.r_flag[a0]) | int(res.r_flag[b0])) & 0x8000:
            continue
        n_unique += 1
        x = insert_of(res, a0, b0, 0, im.INSERT_MAX, orient)
        if x is not None:
            ins.append(x)
    return im.from_inserts(n_pairs, n_unique, ins)


def choice(by):
    """The orientation of three estimates: most informative pairs among the estimated ones, ties in the order FR RF FF; -1."""
    best = -1
    for o in (FR, RF, FF):
        if by[o]["estimated"] and (best < 0 or by[o]["n_informative"] > by[best]["n_informative"]):
            best = o
    return best


def library_estimate(res, n_pairs):
    """fem_dev_estimate_library: dict(by = the three estimates, orientation = the choice)."""
    by = [estimate(res, n_pairs, o) for o in (FR, RF, FF)]
    return dict(by=by, orientation=choice(by))
