"""Plain-Python model of the header lines and tags of FEM map --header / --rg / --nh (fem_dev_set_tags in include/fem_hip.h).

The rule.  The tags are added to lines, after everything else has been decided (order, rescue, pairing, MAPQ, the lines of
unmapped reads, the line filter).  A slot is a read single-end, or one mate of a pair (tests.report_model.slots).  A mapped line
gets NH:i:<the lines of its slot in the text> HI:i:<its 1-based place among them>, then RG:Z:<ID>; the line of an unmapped read
(FLAG & 4) gets RG:Z alone.  In BAM NH and HI are type I (four bytes, whatever the value) and RG is type Z.

Input: a SAM text without header and without these tags, as bytes: what tests.report_model / tests.unmapped_model expect."""
import functools
import struct

import numpy as np

from tests import bam_model as bm
from tests import report_model as rp

HD = b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n"
TAGS = (b"NH", b"HI", b"RG")


def apply(text, read_group=None, hits=False):
    """`text` with RG:Z:<read_group> (bytes; None: none) on every line and, with hits, NH:i HI:i on every mapped one."""
    out = []
    for lines in rp.slots(text):
        mapped = not int(lines[0].split(b"\t", 2)[1]) & 4
        for i, l in enumerate(lines):
            l = l[:-1]
            if hits and mapped:
                l += b"\tNH:i:%d\tHI:i:%d" % (len(lines), i + 1)
            if read_group is not None:
                l += b"\tRG:Z:" + read_group
            out.append(l + b"\n")
    return b"".join(out)


def strip(text):
    """(the text without the three tags, [(NH, HI, RG) per line, None where a line has none])."""
    out, tags = [], []
    for l in text.split(b"\n"):
        if not l:
            continue
        f = l.split(b"\t")
        t = {x[:2]: x[5:] for x in f[11:] if x[:2] in TAGS}
        assert [x[:2] for x in f[11:] if x[:2] in TAGS] == [k for k in TAGS if k in t], l  # their order, each once, behind the others
        assert all(x[:2] not in TAGS for x in f[11:len(f) - len(t)])
        out.append(b"\t".join(f[:len(f) - len(t)]) + b"\n")
        tags.append((int(t[b"NH"]) if b"NH" in t else None, int(t[b"HI"]) if b"HI" in t else None, t.get(b"RG")))
    return b"".join(out), tags


def aux(nh=None, hi=None, read_group=None):
    """The BAM aux bytes of the three tags."""
    out = b""
    if nh is not None:
        out += b"NHI" + struct.pack("<I", nh) + b"HII" + struct.pack("<I", hi)
    if read_group is not None:
        out += b"RGZ" + read_group + b"\0"
    return out


def aux_decode(data):
    """The aux bytes of a record of FEM map -> [(tag, type, value)] (types C, I and Z: NM, NH / HI, MD / RG)."""
    out, p = [], 0
    while p < len(data):
        tag, typ = data[p:p + 2], data[p + 2:p + 3]
        p += 3
        if typ == b"C":
            out.append((tag, typ, data[p]))
            p += 1
        elif typ == b"I":
            out.append((tag, typ, struct.unpack_from("<I", data, p)[0]))
            p += 4
        elif typ == b"Z":
            z = data.index(b"\0", p)
            out.append((tag, typ, data[p:z]))
            p = z + 1
        else:
            raise ValueError("aux type %r not expected" % typ)
    return out


def record_aux(rec):
    """The aux bytes of one BAM record (block_size included)."""
    l_name, = struct.unpack_from("<B", rec, 12)
    n_ops, = struct.unpack_from("<H", rec, 16)
    l_seq, = struct.unpack_from("<i", rec, 20)
    return rec[36 + l_name + 4 * n_ops + (l_seq + 1) // 2 + l_seq:]


def bam_payload(text, ref_names):
    """The BAM records of a tagged SAM text: tests.bam_model's record of each line without the three tags, these behind it."""
    plain, tags = strip(text)
    out = []
    for l, t in zip(plain.split(b"\n"), tags):
        rec, extra = bm.encode(l, ref_names), aux(*t)
        out.append(struct.pack("<i", len(rec) - 4 + len(extra)) + rec[4:] + extra)
    return b"".join(out)


def pg_line(argv, version):
    """The @PG line (no newline) of a command line: argv (list of str) joined by single spaces, a tab inside an argument as the
    two characters \\t, a newline as a space."""
    cl = " ".join(a.replace("\t", "\\t").replace("\n", " ") for a in argv)
    return ("@PG\tID:FEM\tPN:FEM\tVN:%s\tCL:%s" % (version, cl)).encode("latin-1")


def rg_line(arg):
    """The @RG line (no newline) of a valid --rg argument: the two characters \\t are tabs."""
    return arg.replace("\\t", "\t").encode("latin-1")


def header(sq_text, rg=None, pg=None):
    """The header of --header: @HD, the @SQ lines (bytes, as without the switch), the @RG line, the @PG line."""
    return HD + sq_text + b"".join(l + b"\n" for l in (rg, pg) if l is not None)


@functools.lru_cache(maxsize=None)
def asserted_case():
    """A batch whose records include 0x8000 ones (the reference would have asserted: the traceback compares characters, so an
    upper-case read on a lower-case stretch of the reference is verified and then not traced; written with CIGAR * and an empty
    MD): one unit in five spaced copies, two of them in lower case (slots of about five lines, 0x8000 ones among the secondary
    lines), reads from a lower-case stretch (slots whose only line is one), reads that map plainly and reads of random letters."""
    from oracle import fem_oracle as fo
    from tests import util
    rng, L = np.random.default_rng(340), 100
    unit = util.rand_seq(rng, L + 60)
    parts = [util.rand_seq(rng, 3000)]
    for k in range(5):
        parts += [unit.lower() if k in (1, 3) else unit, util.rand_seq(rng, L + 20)]
    low = util.rand_seq(rng, 4000)
    seqs = [b"".join(parts), low[:1000] + low[1000:3000].lower() + low[3000:], util.rand_seq(rng, 20000)]
    reads = [util.mutate(rng, unit[o:o + L], int(rng.integers(0, 3))) for o in rng.integers(0, 61, 6)]
    reads += [util.mutate(rng, seqs[1][s:s + L].upper(), int(rng.integers(0, 4))) for s in rng.integers(1000, 2900, 8)]
    reads += util.make_reads(rng, seqs[2:], 8, L, 2)
    reads += [util.rand_seq(rng, L) for _ in range(4)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=3, threads=4)
    quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
    return dict(seqs=seqs, names=["units", "low", "plain"], reads=reads, rnames=["a%d" % i for i in range(len(reads))], quals=quals, e=3,
                idx=idx, res=res)
