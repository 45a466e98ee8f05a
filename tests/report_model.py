"""Plain-Python model of the line filter (FEM map --strata / --max-hits; fem_dev_set_report in include/fem_hip.h).

The rule.  The filter acts on lines, after everything else has been decided (order, rescue, pairing, MAPQ, the line of an
unmapped read), and only removes lines.  A slot is a read single-end, or one mate of a pair; its lines in output order are
l_0 .. l_{c-1}, l_0 the primary line, and d the least NM over all of them.  l_0 is always kept; a later line l_t is kept iff
(S off or nm(l_t) <= d + S) and (N off or fewer than N lines of the slot have been kept before it, l_0 included).  A line with
FLAG & 4 (an unmapped read's) is a slot of its own.

Input: a SAM text without header, as bytes: the expected text of the other models (tests.unmapped_model's single_end / paired,
which carry the MAPQ of tests.mapq_model and the pairing of tests.pair_model) or the device's own unfiltered text."""
from tests import unmapped_model as um


def slots(text):
    """The lines of `text` (bytes, each with its newline) grouped by slot.  A slot starts at every line that is not a secondary
    one (FLAG & 0x100 clear: a read's, in pair mode a mate's, first line) and at every line with FLAG & 4; the lines of a slot
    share QNAME and the 0x40 / 0x80 bits."""
    out = []
    for l in text.split(b"\n"):
        if not l:
            continue
        f = l.split(b"\t", 2)
        flag = int(f[1])
        if flag & 4 or not flag & 0x100:
            out.append([])
        else:
            first = out[-1][0].split(b"\t", 2)
            assert first[0] == f[0] and (int(first[1]) ^ flag) & 0xC0 == 0 and not int(first[1]) & 4, (first[:2], f[:2])
        out[-1].append(l + b"\n")
    return out


def line_nm(line):
    """NM of a mapped line (its NM:i: tag)."""
    for f in line.rstrip(b"\n").split(b"\t")[11:]:
        if f.startswith(b"NM:i:"):
            return int(f[5:])
    raise ValueError("a line without NM:i: %r" % line[:80])


def keep(nms, strata=None, max_hits=None):
    """Which of a slot's lines stay, from their NM in output order (list of bool)."""
    d = min(nms)
    kept, n = [], 0
    for t, v in enumerate(nms):
        k = t == 0 or ((strata is None or v <= d + strata) and (max_hits is None or n < max_hits))
        kept.append(k)
        n += k
    return kept


def apply(text, strata=None, max_hits=None):
    """(the text the filter leaves of `text`, the number of lines it drops)."""
    out, dropped = [], 0
    for lines in slots(text):
        if int(lines[0].split(b"\t", 2)[1]) & 4:
            out += lines
            continue
        for l, k in zip(lines, keep([line_nm(l) for l in lines], strata, max_hits)):
            if k:
                out.append(l)
            else:
                dropped += 1
    return b"".join(out), dropped


def _with_reads(make, names):
    """make(names) -> (text, dropped), with the read of every line: the text is made under the reads' numbers for names, which
    only column 1 prints, and the names are put back -> (text, dropped, [the read of each line])."""
    text, dropped = make(["%d" % r for r in range(len(names))])
    out, line_reads = [], []
    for l in text.split(b"\n"):
        if l:
            r, rest = l.split(b"\t", 1)
            line_reads.append(int(r))
            out.append(names[int(r)].encode("latin-1") + b"\t" + rest + b"\n")
    return b"".join(out), dropped, line_reads


def single_end(res, seq_names, reads, names, quals, e=None, unmapped=True, strata=None, max_hits=None, with_reads=False):
    """The filtered single-end text from the oracle's records -> (text, dropped).  e: with MAPQ at -e e; unmapped: with the
    unmapped reads' lines; with_reads: -> (text, dropped, the read of each line), for names that repeat."""
    if with_reads:
        return _with_reads(lambda nm: single_end(res, seq_names, reads, nm, quals, e, unmapped, strata, max_hits), names)
    text = um.single_end(res, seq_names, reads, names, quals, e=e)
    if not unmapped:
        text = um.without_unmapped(text)[0]
    return apply(text, strata, max_hits)


def paired(se, n_pairs, seq_names, reads, names, quals, min_insert=0, max_insert=500, res=None, rescued=(), e=None, unmapped=True,
           strata=None, max_hits=None, with_reads=False):
    """The filtered paired text -> (text, dropped); the arguments of unmapped_model.paired, and `unmapped` and `with_reads` as above."""
    if with_reads:
        return _with_reads(lambda nm: paired(se, n_pairs, seq_names, reads, nm, quals, min_insert, max_insert, res, rescued, e, unmapped,
                                             strata, max_hits), names)
    text = um.paired(se, n_pairs, seq_names, reads, names, quals, min_insert, max_insert, res=res, rescued=rescued, e=e)
    if not unmapped:
        text = um.without_unmapped(text, True)[0]
    return apply(text, strata, max_hits)
