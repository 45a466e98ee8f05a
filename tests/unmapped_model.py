"""Plain-Python model of the lines for unmapped reads (FEM map --unmapped; fem_dev_set_unmapped in include/fem_hip.h).

The rule.  A read is unmapped when, after single-end mapping and (pair mode with rescue) after mate rescue, it has no record.
It gets exactly one line where its records would have stood: single-end in batch read order, in pair mode in the pair's slot
(mate 1's lines, then mate 2's).  Mapped reads keep their lines.

The unplaced line (single-end; a pair with both mates unmapped): QNAME, FLAG 4 (pairs 77 and 141), * 0, MAPQ 0, *, * 0 0, SEQ
and QUAL of the read as given (* * for a read of length 0), no tags.
The placed line (pair with a mapped mate A and an unmapped mate B; a0 = A's first line, on sequence t at pos0 p): B's line has
FLAG 0x1 | 0x4 | 0x40 or 0x80 (| 0x20 when a0 is reverse), t, p + 1, MAPQ 0, *, =, p + 1, 0, SEQ, QUAL, no tags; A's lines keep
0x8 and everything else, but RNEXT PNEXT name (t, p + 1): = where the line's own sequence is t, else t's name.

Input: the oracle's single-end records (fo.map_reads) or hand-built tests.pair_model.Records; tests.pair_model for the
pairing, tests.rescue_model's records for rescued lists, tests.mapq_model for the MAPQ of the mapped reads' lines."""
from tests import mapq_model as mq
from tests import pair_model as pm

_IUPAC = "=ACMGRSVTWYHKDBN"


def seq_letters(read):
    """SEQ as every line prints it: the 4-bit round trip of a BAM record (IUPAC letters upper-cased, the digits 0-3 as ACGT,
    anything else N)."""
    out = []
    for c in read:
        ch = chr(c).upper()
        out.append("ACGT"[c - 48] if 48 <= c <= 51 else ch if ch in _IUPAC else "N")
    return "".join(out)


def _seq_qual(read, qual):
    if not len(read):
        return "*", "*"
    return seq_letters(read), "*" if qual is None else qual


def _mapped(res, j, name, flag, seq_names, mapq, rnext, pnext, tlen, read, qual):
    primary = not flag & 256
    seq, q = _seq_qual(read, qual) if primary else ("*", "*")
    return "\t".join([name, str(flag & 0x7FFF), seq_names[int(res.r_tid[j])], str(int(res.r_pos[j]) + 1), str(mapq),
                      res.cigar_str(j) or "*", rnext, str(pnext), str(tlen), seq, q, "NM:i:%d" % int(res.r_nm[j]),
                      "MD:Z:" + res.md_str(j)])


def _unmapped(name, flag, rname, pos1, rnext, read, qual):
    seq, q = _seq_qual(read, qual)
    return "\t".join([name, str(flag), rname, str(pos1), "0", "*", rnext, str(pos1), "0", seq, q])


def _bytes(lines):
    return "".join(l + "\n" for l in lines).encode("latin-1")


def unmapped_reads(res, n_reads):
    return [r for r in range(n_reads) if int(res.rec_off[r + 1]) == int(res.rec_off[r])]


def single_end(res, seq_names, reads, names, quals, e=None):
    """The single-end text with the switch on (bytes).  quals: per read, or None (QUAL *); e: with MAPQ at -e e, None: 255."""
    mapqs = iter(mq.single_end(res, e)) if e is not None else None
    out = []
    for r in range(len(reads)):
        lo, hi = int(res.rec_off[r]), int(res.rec_off[r + 1])
        qual = None if quals is None else quals[r]
        if lo == hi:
            out.append(_unmapped(names[r], 4, "*", 0, "*", reads[r], qual))
        for j in range(lo, hi):  # (the records carry 256 on every line but the read's first)
            mapq = next(mapqs) if mapqs is not None else 255
            out.append(_mapped(res, j, names[r], int(res.r_flag[j]), seq_names, mapq, "*", 0, 0, reads[r], qual))
    return _bytes(out)


def paired(se, n_pairs, seq_names, reads, names, quals, min_insert=0, max_insert=500, res=None, rescued=(), e=None):
    """The paired text with the switch on (bytes).  se: the single-end records; res: the lists pairing sees
    (rescue_model.rescue's records; default se) and rescued the reads whose list is a rescued record; e: with MAPQ, None: 255."""
    res = se if res is None else res
    lines, _ = pm.expected(res, n_pairs, min_insert, max_insert)
    mapqs = mq.paired(se, n_pairs, e, min_insert, max_insert, res=res, rescued=rescued) if e is not None else [255] * len(lines)
    by_read = {}
    for ln, q in zip(lines, mapqs):
        by_read.setdefault(ln[0], []).append((ln, q))
    out = []
    for i in range(n_pairs):
        mates = (i, n_pairs + i)
        for m, r in enumerate(mates):
            mine, other = by_read.get(r, []), by_read.get(mates[1 - m], [])
            qual = None if quals is None else quals[r]
            if not mine:
                flag = 0x1 | 0x4 | (0x80 if m else 0x40)
                if not other:
                    out.append(_unmapped(names[r], flag | 0x8, "*", 0, "*", reads[r], qual))
                else:  # placed at the mapped mate's first line
                    a0 = other[0][0]
                    t, p = int(res.r_tid[a0[1]]), int(res.r_pos[a0[1]])
                    out.append(_unmapped(names[r], flag | (0x20 if a0[2] & 16 else 0), seq_names[t], p + 1, "=", reads[r], qual))
                continue
            for (_, j, flag, mt, mp, tlen), q in mine:
                if not other:  # the mate's line is placed at this read's first line
                    j0 = mine[0][0][1]
                    mt, mp = int(res.r_tid[j0]), int(res.r_pos[j0])
                rnext = "*" if mt is None else "=" if mt == int(res.r_tid[j]) else seq_names[mt]
                out.append(_mapped(res, j, names[r], flag, seq_names, q, rnext, 0 if mt is None else mp + 1, tlen, reads[r], qual))
    return _bytes(out)


def pair_classes(res, n_pairs):
    """How many pairs have (both mates, only mate 1, only mate 2, neither) with a record."""
    n = [0, 0, 0, 0]
    for i in range(n_pairs):
        a = int(res.rec_off[i + 1]) > int(res.rec_off[i])
        b = int(res.rec_off[n_pairs + i + 1]) > int(res.rec_off[n_pairs + i])
        n[0 if a and b else 1 if a else 2 if b else 3] += 1
    return n


def without_unmapped(text, paired_mode=False):
    """A text made with the switch on, as bytes, minus its lines with FLAG & 4 (pairs: and * 0 back in columns 7-8 of the
    lines that carry 0x8) -> (the text, the number of lines removed)."""
    out, removed = [], 0
    for l in text.split(b"\n"):
        if not l:
            continue
        f = l.split(b"\t")
        flag = int(f[1])
        if flag & 4:
            removed += 1
            continue
        if paired_mode and flag & 8:
            f[6], f[7] = b"*", b"0"
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out), removed
