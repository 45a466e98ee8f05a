"""Plain-Python model of the mate tags of FEM map --mate-tags (fem_dev_set_mate_tags in include/fem_hip.h).

The rule.  A paired text's lines come slot by slot (tests.report_model.slots): mate 1 of a pair (FLAG & 0x40), then mate 2
(FLAG & 0x80).  The other mate's primary line is the first line of its slot, unless that is the line of an unmapped read
(FLAG & 4), which is no record.  Every line of a slot gets, behind everything it has:
  MC:Z:<the other mate's primary line's CIGAR column>   iff the other mate has a record and that column is not "*";
  MQ:i:<that line's MAPQ column>                        iff the other mate has a record;
  ms:i:<the sum of b - 33 over the other mate's quality bytes b with b - 33 >= 15>   iff the batch has qualities.
In BAM MC is type Z, MQ type C and ms type I (four bytes, whatever the value).

Input: a paired SAM text without header and without these tags, as bytes (with or without the tags of tests.tags_model: the
mate tags come last, so apply() composes behind tags_model.apply), and the qualities of the batch's 2 * n_pairs reads in batch
order (read i and read n_pairs + i are pair i): a mate without a record has no line to read them from unless the text has the
lines of unmapped reads.  The pairs of the text are found among the batch's by the QUAL column of their primary lines, in order
(so two neighbouring pairs that share a name must not share their qualities too)."""
import struct

from tests import bam_model as bm
from tests import report_model as rp
from tests import tags_model as tm

TAGS = (b"MC", b"MQ", b"ms")
MIN_QUAL = 15


def score(qual):
    """ms of a mate with these quality characters (bytes)."""
    return sum(b - 33 for b in bytes(qual) if b - 33 >= MIN_QUAL)


def pairs(text):
    """The slots of `text` grouped by pair: [[mate 1's lines or None, mate 2's lines or None]]."""
    out = []
    for lines in rp.slots(text):
        f = lines[0].split(b"\t", 2)
        flag = int(f[1])
        assert flag & 1 and bool(flag & 0x40) != bool(flag & 0x80), lines[0]
        m = 1 if flag & 0x80 else 0
        if m == 1 and out and out[-1][1] is None and out[-1][0] is not None and out[-1][0][0].split(b"\t", 1)[0] == f[0]:
            out[-1][1] = lines
        else:
            out.append([None, None])
            out[-1][m] = lines
    return out


def apply(text, n_pairs, quals):
    """`text` with MC:Z, MQ:i and ms:i on every line.  quals: list of 2 * n_pairs str / bytes, or None: reads without qualities
    (QUAL prints *), no ms."""
    if quals is not None:
        quals = [q.encode("latin-1") if isinstance(q, str) else bytes(q) for q in quals]
        assert len(quals) == 2 * n_pairs
    out, at = [], 0
    for pair in pairs(text):
        ms = [None, None]  # of mate 1 and of mate 2
        if quals is not None:
            def is_pair(i):
                for m, lines in enumerate(pair):
                    if lines is not None and lines[0][:-1].split(b"\t")[10] != (quals[m * n_pairs + i] or b"*"):
                        return False
                return True
            while at < n_pairs and not is_pair(at):
                at += 1
            assert at < n_pairs, "a pair of the text is none of the batch's: %r" % (pair,)
            ms = [score(quals[at]), score(quals[n_pairs + at])]
            at += 1
        for m, lines in enumerate(pair):
            other = pair[m ^ 1]
            tags = b""
            if other is not None and not int(other[0].split(b"\t", 2)[1]) & 4:
                f = other[0].split(b"\t")
                if f[5] != b"*":
                    tags += b"\tMC:Z:" + f[5]
                tags += b"\tMQ:i:" + f[4]
            if ms[m ^ 1] is not None:
                tags += b"\tms:i:%d" % ms[m ^ 1]
            for l in lines or []:
                out.append(l[:-1] + tags + b"\n")
    return b"".join(out)


def strip(text):
    """(the text without the three tags, [(MC, MQ, ms) per line, None where a line has none])."""
    out, tags = [], []
    for l in text.split(b"\n"):
        if not l:
            continue
        f = l.split(b"\t")
        t = {x[:2]: x[5:] for x in f[11:] if x[:2] in TAGS}
        assert [x[:2] for x in f[11:] if x[:2] in TAGS] == [k for k in TAGS if k in t], l  # their order, each once ...
        assert all(x[:2] not in TAGS for x in f[11:len(f) - len(t)]), l                      # ... behind every other field
        out.append(b"\t".join(f[:len(f) - len(t)]) + b"\n")
        tags.append((t.get(b"MC"), int(t[b"MQ"]) if b"MQ" in t else None, int(t[b"ms"]) if b"ms" in t else None))
    return b"".join(out), tags


def aux(mc=None, mq=None, ms=None):
    """The BAM aux bytes of the three tags."""
    out = b""
    if mc is not None:
        out += b"MCZ" + mc + b"\0"
    if mq is not None:
        out += b"MQC" + struct.pack("<B", mq)
    if ms is not None:
        out += b"msI" + struct.pack("<I", ms)
    return out


def aux_decode(data):
    """The aux bytes of a record -> [(tag, type, value)] (tests.tags_model.aux_decode: types C, I and Z cover MQ, ms and MC)."""
    return tm.aux_decode(data)


def record_tags(rec):
    """(MC, MQ, ms) of one BAM record, None where it has none; asserts their types and that they stand last, in order."""
    fields = aux_decode(tm.record_aux(rec))
    mine = [(t, typ, v) for t, typ, v in fields if t in TAGS]
    assert fields[len(fields) - len(mine):] == mine and [t for t, _, _ in mine] == [k for k in TAGS if k in dict((t, 0) for t, _, _ in mine)]
    assert all(typ == {b"MC": b"Z", b"MQ": b"C", b"ms": b"I"}[t] for t, typ, _ in mine)
    got = {t: v for t, _, v in mine}
    return got.get(b"MC"), got.get(b"MQ"), got.get(b"ms")


def bam_payload(text, ref_names):
    """The BAM records of a SAM text with mate tags: tests.tags_model's record of each line without them, these behind it."""
    plain, tags = strip(text)
    out = []
    for rec, t in zip(bm.records(tm.bam_payload(plain, ref_names)), tags):
        extra = aux(*t)
        out.append(struct.pack("<i", len(rec) - 4 + len(extra)) + rec[4:] + extra)
    return b"".join(out)
