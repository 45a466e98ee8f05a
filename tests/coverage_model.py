"""The rule of the coverage track (include/fem_hip.h, fem_dev_set_coverage) in plain Python, computed from SAM text alone: the
lines' FLAG, RNAME, POS, MAPQ and CIGAR columns, and with all_hits the entries of XA:Z.  Because it reads the text, the device's
own output under any combination of options is its input, and it knows nothing of the kernel's view of records.  The one thing
the text cannot show is the MAPQ of a line that XA folded away (an entry carries none): with min_mapq > 0 the caller hands in the
text of the same batch rendered without XA; folding never changes the track.

The depth is taken base by base (a difference array per sequence) and summed into windows afterwards, so the windows' arithmetic
is not the kernel's either."""
import re

import numpy as np

_OPS = re.compile(rb"(\d+)([MIDNSHP=X])")


def span(cigar):
    """The reference bases a CIGAR column covers under the rule: the M and D lengths (S and I are passed over); None for *."""
    if cigar == b"*":
        return None
    ops = _OPS.findall(cigar)
    assert ops and b"".join(n + o for n, o in ops) == cigar, cigar
    return sum(int(n) for n, o in ops if o in (b"M", b"D"))


def lines(text):
    """The alignment lines of a SAM text (bytes) -> [(flag, rname, pos0, mapq, cigar, [(rname, pos0, cigar) of XA:Z])]."""
    out = []
    for l in text.split(b"\n"):
        if not l or l.startswith(b"@"):
            continue
        f = l.split(b"\t")
        xa = []
        for t in f[11:]:
            if t.startswith(b"XA:Z:"):
                for e in t[5:].split(b";"):
                    if e:
                        rname, pos, cigar, _nm = e.split(b",")
                        xa.append((rname, int(pos[1:]) - 1, cigar))
        out.append((int(f[1]), f[2], int(f[3]) - 1, int(f[4]), f[5], xa))
    return out


def counting(text, all_hits=False, min_mapq=0):
    """The (rname, pos0, span) of everything that counts under rule 1, in text order."""
    out = []
    for flag, rname, pos0, mapq, cigar, xa in lines(text):
        assert not (xa and all_hits and min_mapq > 0), "an XA entry carries no MAPQ: hand in the text rendered without XA"
        if not flag & 4 and (all_hits or not flag & 0x100) and span(cigar) is not None and mapq >= min_mapq:
            out.append((rname, pos0, span(cigar)))
        if all_hits:  # (the entries stand on the slot's first line whether or not that line itself counts)
            out += [(r, p, span(c)) for r, p, c in xa if span(c) is not None]
    return out


def layout(seq_lens, window):
    """bin_off (n_seq + 1 entries): a sequence of n bases has ceil(n / window) windows."""
    off = [0]
    for n in seq_lens:
        off.append(off[-1] + -(-int(n) // window))
    return off


def bins(text, names, seq_lens, window, all_hits=False, min_mapq=0):
    """The track of one text: uint64 bins in the order of the sequences, then position.  names: bytes or str, as in @SQ."""
    tid = {(n.encode() if isinstance(n, str) else bytes(n)): t for t, n in enumerate(names)}
    diff = [np.zeros(int(n) + 1, np.int64) for n in seq_lens]
    for rname, pos0, s in counting(text, all_hits, min_mapq):
        d = diff[tid[rname]]
        lo, hi = min(pos0, len(d) - 1), min(pos0 + s, len(d) - 1)  # (a span is cut at its sequence's end)
        d[lo] += 1
        d[hi] -= 1
    out = []
    for d in diff:
        depth = np.cumsum(d[:-1])
        if len(depth):
            out.append(np.add.reduceat(depth, np.arange(0, len(depth), window)))
    return np.concatenate(out).astype(np.uint64) if out else np.zeros(0, np.uint64)


def bed(names, seq_lens, window, track):
    """The BED text of a track, by the format of fem_coverage_write: name, start, end, bases, mean with two decimals in integers."""
    out, k = [], 0
    for name, n in zip(names, seq_lens):
        name = name.encode() if isinstance(name, str) else bytes(name)
        for start in range(0, int(n), window):
            end = min(start + window, int(n))
            b, ln = int(track[k]), end - start
            h = (b * 100 + ln // 2) // ln
            out.append(b"%s\t%d\t%d\t%d\t%d.%02d\n" % (name, start, end, b, h // 100, h % 100))
            k += 1
    assert k == len(track)
    return b"".join(out)
