"""Plain-Python model of paired-end output (FEM map --read2; fem_dev_set_pairs in include/fem_hip.h).

Input: the single-end records of a batch of 2 n reads, pair i being read i (mate 1) and read n + i (mate 2), in the form
fo.map_reads returns them (rec_off, r_flag, r_tid, r_pos, r_nm, cig_off, cig, md_off, md).  Output: the chosen combination
of every pair, the expected SAM lines and the expected fem_batch_pairs arrays."""
import numpy as np


class Records:
    """Hand-built single-end records with the fields of fo.MapResult (for the model's own tests)."""

    def __init__(self, per_read):
        """per_read: one list per read of (flag, tid, pos0, nm, cigar [(len, op)], md) tuples, op in "MID"."""
        self.rec_off = np.zeros(len(per_read) + 1, np.uint64)
        self.rec_off[1:] = np.cumsum([len(r) for r in per_read])
        recs = [x for r in per_read for x in r]
        self.r_flag = np.array([x[0] for x in recs], np.uint16)
        self.r_tid = np.array([x[1] for x in recs], np.uint32)
        self.r_pos = np.array([x[2] for x in recs], np.uint32)
        self.r_nm = np.array([x[3] for x in recs], np.uint8)
        self.cig_off = np.zeros(len(recs) + 1, np.uint64)
        self.cig_off[1:] = np.cumsum([len(x[4]) for x in recs])
        self.cig = np.array([n << 4 | "MID".index(o) for x in recs for n, o in x[4]], np.uint32)
        self.md_off = np.zeros(len(recs) + 1, np.uint64)
        self.md_off[1:] = np.cumsum([len(x[5]) for x in recs])
        self.md = np.frombuffer("".join(x[5] for x in recs).encode(), np.uint8)

    def cigar_str(self, j):
        ops = self.cig[int(self.cig_off[j]):int(self.cig_off[j + 1])]
        return "".join("%d%s" % (int(o) >> 4, "MID"[int(o) & 0xF]) for o in ops)

    def md_str(self, j):
        return self.md[int(self.md_off[j]):int(self.md_off[j + 1])].tobytes().decode()


def span(res, j):
    ops = res.cig[int(res.cig_off[j]):int(res.cig_off[j + 1])]
    return sum(int(o) >> 4 for o in ops if int(o) & 0xF in (0, 2))


def insert_of(res, ja, jb, min_insert, max_insert):
    """The insert of records ja, jb if the combination is concordant, else None."""
    fa, fb = int(res.r_flag[ja]), int(res.r_flag[jb])
    if (fa | fb) & 0x8000 or int(res.r_tid[ja]) != int(res.r_tid[jb]) or not (fa ^ fb) & 16:
        return None
    f, r = (jb, ja) if fa & 16 else (ja, jb)
    if int(res.r_pos[f]) > int(res.r_pos[r]):
        return None
    ins = int(res.r_pos[r]) + span(res, r) - int(res.r_pos[f])
    return ins if min_insert <= ins <= max_insert else None


def choose(res, n_pairs, min_insert, max_insert):
    """Per pair: (index a, index b, insert) of the chosen combination, or None."""
    out = []
    for i in range(n_pairs):
        a0, a1 = int(res.rec_off[i]), int(res.rec_off[i + 1])
        b0, b1 = int(res.rec_off[n_pairs + i]), int(res.rec_off[n_pairs + i + 1])
        best = None
        if a1 > a0 and b1 > b0:
            # vectorised over B for long lists (repeat-rich references give thousands of records per mate)
            bj = np.arange(b0, b1)
            b_flag = res.r_flag[b0:b1].astype(np.int64)
            b_tid = res.r_tid[b0:b1].astype(np.int64)
            b_pos = res.r_pos[b0:b1].astype(np.int64)
            b_nm = res.r_nm[b0:b1].astype(np.int64)
            b_end = b_pos + np.array([span(res, j) for j in bj], np.int64)
            for a in range(a1 - a0):
                ja = a0 + a
                fa = int(res.r_flag[ja])
                if fa & 0x8000:
                    continue
                pa, ea = int(res.r_pos[ja]), int(res.r_pos[ja]) + span(res, ja)
                ok = ((b_flag & 0x8000) == 0) & (b_tid == int(res.r_tid[ja])) & (((b_flag ^ fa) & 16) != 0)
                if fa & 16:  # a reverse, b forward
                    ins = ea - b_pos
                    ok &= b_pos <= pa
                else:
                    ins = b_end - pa
                    ok &= pa <= b_pos
                ok &= (ins >= min_insert) & (ins <= max_insert)
                if not ok.any():
                    continue
                s = np.where(ok, b_nm + int(res.r_nm[ja]), 1 << 30)
                b = int(np.argmin(s))  # first index of the least sum
                if best is None or int(s[b]) < best[3]:
                    best = (a, b, int(ins[b]), int(s[b]))
        out.append(None if best is None else best[:3])
    return out


def line_order(res, n_pairs, chosen):
    """Per pair and mate: the record numbers of its lines, in output order."""
    order = []
    for i in range(n_pairs):
        for m, r in ((0, i), (1, n_pairs + i)):
            lo, hi = int(res.rec_off[r]), int(res.rec_off[r + 1])
            recs = list(range(lo, hi))
            if chosen[i] is not None:
                c = lo + chosen[i][m]
                recs = [c] + [j for j in recs if j != c]
            order.append(recs)
    return order


def expected(res, n_pairs, min_insert=0, max_insert=500):
    """(per-line tuples, n_proper): each line (read, record, flag with 0x8000 kept, mate_tid or None, mate_pos0, tlen),
    mate 1's lines then mate 2's for every pair."""
    chosen = choose(res, n_pairs, min_insert, max_insert)
    order = line_order(res, n_pairs, chosen)
    lines = []
    for i in range(n_pairs):
        c = chosen[i]
        for m in (0, 1):
            recs, other = order[2 * i + m], order[2 * i + 1 - m]
            r = i if m == 0 else n_pairs + i
            o = other[0] if other else None
            for t, j in enumerate(recs):
                fl = int(res.r_flag[j])
                flag = (fl & 0x8010) | 0x1 | (0x80 if m else 0x40) | (256 if t else 0)
                if c is not None and t == 0:
                    flag |= 0x2
                if o is None:
                    flag |= 0x8
                elif int(res.r_flag[o]) & 16:
                    flag |= 0x20
                tlen = 0
                if c is not None and t == 0:
                    tlen = -c[2] if fl & 16 else c[2]
                lines.append((r, j, flag, None if o is None else int(res.r_tid[o]), None if o is None else int(res.r_pos[o]),
                              tlen))
    return lines, sum(x is not None for x in chosen)


def sam_lines(res, n_pairs, seq_names, reads, names, quals, min_insert=0, max_insert=500):
    """The expected paired SAM text (names already without /1 /2; reads and quals as staged, 2 n_pairs of each)."""
    lines, _ = expected(res, n_pairs, min_insert, max_insert)
    out = []
    for r, j, flag, mt, mp, tlen in lines:
        primary = not flag & 256
        tid = int(res.r_tid[j])
        rnext = "*" if mt is None else "=" if mt == tid else seq_names[mt]
        cig = res.cigar_str(j) or "*"
        seq = reads[r].decode("latin-1").upper() if primary else "*"
        out.append("\t".join([names[r], str(flag & 0x7FFF), seq_names[tid], str(int(res.r_pos[j]) + 1), "255", cig, rnext,
                              "0" if mt is None else str(mp + 1), str(tlen), seq, quals[r] if primary else "*",
                              "NM:i:%d" % int(res.r_nm[j]), "MD:Z:" + res.md_str(j)]))
    return "".join(l + "\n" for l in out)


def pair_arrays(res, n_pairs, min_insert=0, max_insert=500):
    """The expected fem_batch_pairs arrays (dict of numpy arrays, as fem_amd.device.BatchPairs holds them)."""
    lines, n_proper = expected(res, n_pairs, min_insert, max_insert)
    chosen = choose(res, n_pairs, min_insert, max_insert)
    order = line_order(res, n_pairs, chosen)
    rec_begin = np.zeros(2 * n_pairs + 1, np.uint32)
    rec_begin[1:] = np.cumsum([len(o) for o in order])
    js = np.array([x[1] for x in lines], np.int64)
    cig = [res.cig[int(res.cig_off[j]):int(res.cig_off[j + 1])] for j in js]
    md = [res.md[int(res.md_off[j]):int(res.md_off[j + 1])] for j in js]
    none = 0xFFFFFFFF
    return dict(
        rec_begin=rec_begin,
        flag=np.array([x[2] for x in lines], np.uint16),
        tid=res.r_tid[js].astype(np.uint32) if len(js) else np.zeros(0, np.uint32),
        pos0=res.r_pos[js].astype(np.uint32) if len(js) else np.zeros(0, np.uint32),
        nm=res.r_nm[js].astype(np.uint8) if len(js) else np.zeros(0, np.uint8),
        cigar_off=np.concatenate([[0], np.cumsum([len(c) for c in cig])]).astype(np.uint32),
        cigar=np.concatenate(cig).astype(np.uint32) if cig else np.zeros(0, np.uint32),
        md_off=np.concatenate([[0], np.cumsum([len(m) for m in md])]).astype(np.uint32),
        md=np.concatenate(md).astype(np.uint8) if md else np.zeros(0, np.uint8),
        mate_tid=np.array([none if x[3] is None else x[3] for x in lines], np.uint32),
        mate_pos0=np.array([none if x[4] is None else x[4] for x in lines], np.uint32),
        tlen=np.array([x[5] for x in lines], np.int32),
        n_proper=n_proper)


def strip_mate_suffix(name):
    """QNAME of a mate: the name with a trailing /1 or /2 removed."""
    return name[:-2] if len(name) >= 2 and name[-2] == "/" and name[-1] in "12" else name
