"""The model of the mate tags (tests/mate_tags_model.py) against lines written out by hand: one line of each shape, the
composition behind tests.tags_model.apply, the BAM aux bytes, and that the comparison notices each tag's absence or change."""
import struct

import pytest

from tests import bam_model as bm
from tests import mate_tags_model as mt
from tests import tags_model as tm

# qualities: '0' is 48 (15, the least that counts), '/' is 47 (14: nothing), 'I' is 73 (40)
Q = {"a1": b"II0/", "a2": b"0000", "b1": b"////", "b2": b"I!I~", "c1": b"IIII", "c2": b"0/0/", "d1": b"!!!!", "d2": b"~~~~",
     "e1": b"I0I0", "e2": b"0I0I"}
MS = {"a1": 95, "a2": 60, "b1": 0, "b2": 173, "c1": 160, "c2": 30, "d1": 0, "d2": 372, "e1": 110, "e2": 110}


def _line(name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, qual, tags=b"NM:i:0\tMD:Z:4"):
    f = [name, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"%d" % pnext, b"%d" % tlen, b"ACGT" if qual else b"*",
         qual or b"*"]
    return b"\t".join(f + ([tags] if tags else [])) + b"\n"


def _plain(unmapped=True):
    """Five pairs: a proper one whose mate 2 has a secondary line; mates on two sequences; mate 2 unmapped (with its placed
    line, or without); nothing maps (lines only with `unmapped`); mate 1's primary record prints CIGAR *."""
    t = [_line(b"a", 99, b"chr1", 100, 40, b"4M", b"=", 300, 204, Q["a1"]),
         _line(b"a", 147, b"chr1", 300, 17, b"2M1I1M", b"=", 100, -204, Q["a2"], b"NM:i:1\tMD:Z:3"),
         _line(b"a", 401, b"chr1", 900, 0, b"4M", b"=", 100, 0, b""),
         _line(b"b", 65, b"chr1", 500, 255, b"1M1D3M", b"chr2", 7, 0, Q["b1"], b"NM:i:1\tMD:Z:1^A3"),
         _line(b"b", 145, b"chr2", 7, 3, b"4M", b"chr1", 500, 0, Q["b2"]),
         _line(b"c", 73, b"chr2", 50, 9, b"3M1I", b"=", 50, 0, Q["c1"], b"NM:i:1\tMD:Z:3")]
    if unmapped:
        t.append(_line(b"c", 133, b"chr2", 50, 0, b"*", b"=", 50, 0, Q["c2"], b""))
        t += [_line(b"d", 77, b"*", 0, 0, b"*", b"*", 0, 0, Q["d1"], b""), _line(b"d", 141, b"*", 0, 0, b"*", b"*", 0, 0, Q["d2"], b"")]
    t += [_line(b"e", 65, b"chr1", 700, 12, b"*", b"=", 720, 0, Q["e1"], b"NM:i:0\tMD:Z:"),
          _line(b"e", 129, b"chr1", 720, 30, b"4M", b"=", 700, 0, Q["e2"])]
    return b"".join(t)


QUALS = [Q[p + "1"] for p in "abcde"] + [Q[p + "2"] for p in "abcde"]


def _tags(text):
    return [l.split(b"\t")[11:] for l in text.splitlines()]


def test_score_counts_the_bytes_from_48_on():
    assert {k: mt.score(v) for k, v in Q.items()} == MS
    assert mt.score(b"") == 0 and mt.score(b"/") == 0 and mt.score(b"0") == 15 and mt.score(b"~") == 93


def test_every_shape_of_line_by_hand():
    got = _tags(mt.apply(_plain(), 5, QUALS))
    assert got == [
        [b"NM:i:0", b"MD:Z:4", b"MC:Z:2M1I1M", b"MQ:i:17", b"ms:i:60"],       # proper pair, mate 1
        [b"NM:i:1", b"MD:Z:3", b"MC:Z:4M", b"MQ:i:40", b"ms:i:95"],           # ... mate 2: its primary line
        [b"NM:i:0", b"MD:Z:4", b"MC:Z:4M", b"MQ:i:40", b"ms:i:95"],           # ... and its secondary one, tagged alike
        [b"NM:i:1", b"MD:Z:1^A3", b"MC:Z:4M", b"MQ:i:3", b"ms:i:173"],        # the mate on another sequence
        [b"NM:i:0", b"MD:Z:4", b"MC:Z:1M1D3M", b"MQ:i:255", b"ms:i:0"],
        [b"NM:i:1", b"MD:Z:3", b"ms:i:30"],                                   # the mate unmapped: its score alone
        [b"MC:Z:3M1I", b"MQ:i:9", b"ms:i:160"],                               # ... and its placed line, behind QUAL
        [b"ms:i:372"], [b"ms:i:0"],                                           # a pair of which nothing maps
        [b"NM:i:0", b"MD:Z:", b"MC:Z:4M", b"MQ:i:30", b"ms:i:110"],
        [b"NM:i:0", b"MD:Z:4", b"MQ:i:12", b"ms:i:110"],                      # the mate's primary line prints CIGAR *: no MC
    ]


def test_without_the_lines_of_unmapped_reads_the_qualities_come_from_the_batch():
    with_lines, without = mt.apply(_plain(), 5, QUALS), mt.apply(_plain(False), 5, QUALS)
    keep = [l for l in with_lines.splitlines() if not int(l.split(b"\t")[1]) & 4]
    assert without.splitlines() == keep  # (pair d has no line at all; pair c's mapped mate still has its mate's ms)
    assert [b"NM:i:1", b"MD:Z:3", b"ms:i:30"] in _tags(without)


def test_no_qualities_no_ms():
    plain = b"".join(b"\t".join(l.split(b"\t")[:10] + [b"*"] + l.rstrip(b"\n").split(b"\t")[11:]) + b"\n" for l in _plain().splitlines())
    got, want = _tags(mt.apply(plain, 5, None)), _tags(mt.apply(_plain(), 5, QUALS))
    assert got == [[t for t in line if not t.startswith(b"ms:")] for line in want]
    assert not any(t.startswith(b"ms:") for line in got for t in line) and any(t.startswith(b"MC:") for line in got for t in line)


def test_composes_behind_the_other_tags():
    tagged = tm.apply(_plain(), b"grp1", True)
    got = mt.apply(tagged, 5, QUALS)
    assert _tags(got)[2] == [b"NM:i:0", b"MD:Z:4", b"NH:i:2", b"HI:i:2", b"RG:Z:grp1", b"MC:Z:4M", b"MQ:i:40", b"ms:i:95"]
    assert _tags(got)[6] == [b"RG:Z:grp1", b"MC:Z:3M1I", b"MQ:i:9", b"ms:i:160"]
    assert _tags(got)[7] == [b"RG:Z:grp1", b"ms:i:372"]
    plain, tags = mt.strip(got)
    assert plain == tagged and tags[0] == (b"2M1I1M", 17, 60) and tags[5] == (None, None, 30) and tags[-1] == (None, 12, 110)
    assert tm.strip(plain)[0] == _plain()


def test_bam_aux_bytes_and_their_decoding():
    assert mt.aux(b"2M1I1M", 17, 60) == b"MCZ2M1I1M\0MQC\x11msI\x3c\0\0\0"
    assert mt.aux(None, 255, 0) == b"MQC\xffmsI\0\0\0\0" and mt.aux(None, None, 372) == b"msI\x74\x01\0\0" and mt.aux() == b""
    assert mt.aux_decode(mt.aux(b"4M", 3, 173)) == [(b"MC", b"Z", b"4M"), (b"MQ", b"C", 3), (b"ms", b"I", 173)]
    names = [b"chr1", b"chr2"]
    text = mt.apply(tm.apply(_plain(), b"grp1", True), 5, QUALS)
    payload = mt.bam_payload(text, names)
    recs = bm.records(payload)
    assert len(recs) == text.count(b"\n")
    assert bm.bam_payload_to_sam(payload, names) == text  # block_size includes the tags; every record decodes to its line
    assert [mt.record_tags(r) for r in recs] == mt.strip(text)[1]
    assert recs[0].endswith(b"RGZgrp1\0MCZ2M1I1M\0MQC\x11msI\x3c\0\0\0")
    assert struct.unpack_from("<i", recs[0], 0)[0] == len(recs[0]) - 4


@pytest.mark.parametrize("tag", [b"MC", b"MQ", b"ms"])
def test_a_missing_or_changed_tag_is_noticed(tag):
    want = mt.apply(_plain(), 5, QUALS)
    lines = want.splitlines()
    at = next(i for i, l in enumerate(lines) if b"\t" + tag + b":" in l)
    f = lines[at].split(b"\t")
    k = next(i for i, x in enumerate(f) if x.startswith(tag + b":"))
    missing = lines[:at] + [b"\t".join(f[:k] + f[k + 1:])] + lines[at + 1:]
    changed = lines[:at] + [b"\t".join(f[:k] + [f[k][:5] + (b"5M" if tag == b"MC" else b"%d" % (int(f[k][5:]) + 1))] + f[k + 1:])] + lines[at + 1:]
    assert missing != lines and changed != lines
    assert mt.strip(b"\n".join(missing) + b"\n")[1] != mt.strip(want)[1] and mt.strip(b"\n".join(changed) + b"\n")[1] != mt.strip(want)[1]
    names = [b"chr1", b"chr2"]
    assert mt.bam_payload(b"\n".join(changed) + b"\n", names) != mt.bam_payload(want, names)
    swapped = lines[:at] + [b"\t".join(f[:k] + f[k + 1:] + [f[k]])] + lines[at + 1:]
    if swapped != lines:  # out of order: strip() refuses it
        with pytest.raises(AssertionError):
            mt.strip(b"\n".join(swapped) + b"\n")
