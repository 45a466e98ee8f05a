"""FEM map --sam-seq / fem_dev_set_sam_seq, the parts that need no GPU: the rule of tests/sam_seq_model.py on hand-written lines,
its letter table against the 4-bit codes, SEQ read against CIGAR and NM on the oracle's texts, what the GPU test's case
generators reach, the command line's switch and refusals, the ABI's new symbol."""
import ctypes
import os

import numpy as np
import pytest

from tests import bam_model as bm
from tests import sam_seq_model as m
from tests.harness import ROOT, run_fem

BASE = ("map", "--ref", "a", "--index", "b", "--read1", "c", "-o", "d")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def line(flag, seq, qual, name=b"r", cigar=b"4M", tags=(b"NM:i:0", b"MD:Z:4")):
    return b"\t".join((name, b"%d" % flag, b"chr0", b"7", b"255", cigar, b"*", b"0", b"0", seq, qual) + tuple(tags)) + b"\n"


# ---- the rule on hand-written lines ----

def test_a_forward_line_is_unchanged():
    t = line(0, b"ACGT", b"!#%'")
    assert m.apply(t) == t


def test_a_reverse_line_is_turned():
    assert m.apply(line(16, b"AACGT", b"!#%')")) == line(16, b"ACGTT", b")'%#!")
    # in a paired text: the primary line of a mate, a rescued mate's, a record the reference would have asserted on
    for flag in (83, 147, 16 | 1 | 0x80, 16 | 1 | 0x40 | 8):
        assert m.apply(line(flag, b"AACGT", b"!#%')")) == line(flag, b"ACGTT", b")'%#!")
    assert m.apply(line(16, b"AACGT", b"!#%')", cigar=b"*", tags=(b"NM:i:0", b"MD:Z:"))) == line(16, b"ACGTT", b")'%#!", cigar=b"*", tags=(b"NM:i:0", b"MD:Z:"))


def test_secondary_and_unmapped_lines_are_unchanged():
    for t in (line(16 | 256, b"*", b"*"), line(256, b"*", b"*"), line(1 | 16 | 256 | 0x40, b"*", b"*"),
              line(4, b"AACGT", b"!#%')", cigar=b"*", tags=()),                   # unmapped
              line(1 | 4 | 8 | 0x40, b"AACGT", b"!#%')", cigar=b"*", tags=()),    # a pair of which nothing maps
              line(1 | 4 | 0x20 | 0x80, b"AACGT", b"!#%')", cigar=b"*", tags=(b"RG:Z:x",))):  # placed at a reversed mate: 0x20, no 0x10
        assert m.apply(t) == t


def test_no_qualities_length_one_odd_length_and_tags():
    assert m.apply(line(16, b"AACGT", b"*")) == line(16, b"ACGTT", b"*")
    assert m.apply(line(16, b"*", b"*")) == line(16, b"*", b"*")  # a read of length 0
    assert m.apply(line(16, b"C", b"I", cigar=b"1M")) == line(16, b"G", b"I", cigar=b"1M")
    assert m.apply(line(16, b"ACC", b"abc", cigar=b"3M")) == line(16, b"GGT", b"cba", cigar=b"3M")
    tags = (b"NM:i:1", b"MD:Z:1A2", b"NH:i:2", b"HI:i:1", b"RG:Z:ACGT", b"MC:Z:4M", b"MQ:i:60", b"ms:i:120")
    assert m.apply(line(83, b"AACG", b"!#%'", tags=tags)) == line(83, b"CGTT", b"'%#!", tags=tags)


def test_header_lines_and_line_ends_stay():
    t = b"@HD\tVN:1.6\n@SQ\tSN:chr0\tLN:16\n" + line(16, b"AACG", b"!#%'") + line(0, b"AACG", b"!#%'")
    got = m.apply(t)
    assert got.startswith(b"@HD\tVN:1.6\n@SQ\tSN:chr0\tLN:16\n") and len(got) == len(t) and got.endswith(b"\n")
    assert m.apply(b"") == b""


def test_every_letter():
    seq = m.LETTERS.encode()
    want = m.COMPLEMENT.encode()[::-1]
    assert m.apply(line(16, seq, b"*", cigar=b"16M")) == line(16, want, b"*", cigar=b"16M")
    # what no line prints goes through the letter table first: a -> A -> T, . -> N -> N
    assert m.revcomp(b"a") == b"T" and m.revcomp(b".") == b"N" and m.revcomp(b"-*x") == b"NNN" and m.revcomp(b"ry") == b"RY"


def test_the_rule_is_an_involution():
    rng = np.random.default_rng(5)
    t = bm.synthetic_sam(rng, 200, 75, "illumina")
    assert len(m.turned(t)) >= 20
    assert m.apply(t) != t and m.apply(m.apply(t)) == t
    for cs in m.NM_CASES[:1]:
        t = m.expected(m.nm_case(*cs))
        assert m.apply(m.apply(t)) == t
    t = m.expected(m.letters_case())
    assert m.apply(m.apply(t)) == t


def test_the_table_is_the_codes_bits_reversed():
    assert m.LETTERS.encode() == bm.SEQ_CODES
    for code, (a, b) in enumerate(zip(m.LETTERS, m.COMPLEMENT)):
        rev = int("{:04b}".format(code)[::-1], 2)
        assert m.LETTERS[rev] == b, (code, a, b)
    assert sorted(m.COMPLEMENT) == sorted(m.LETTERS)
    assert all(m.COMPLEMENT[m.LETTERS.index(b)] == a for a, b in zip(m.LETTERS, m.COMPLEMENT))  # its own inverse


def test_bam_of_a_turned_line():
    # byte k holds positions 2k and 2k + 1 of the reversed read; the low nibble of an odd L's last byte is 0
    on = m.apply(line(16, b"ACC", b"abc", cigar=b"3M"))
    rec = bm.records(bm.sam_to_bam_payload(on, [b"chr0"]))[0]
    l_name, n_ops, l_seq = rec[12], rec[16] | rec[17] << 8, int.from_bytes(rec[20:24], "little")
    at = 36 + l_name + 4 * n_ops
    assert l_seq == 3 and rec[at:at + 2] == bytes([0x44, 0x80]) and rec[at + 2:at + 5] == bytes([ord(c) - 33 for c in "cba"])


# ---- SEQ read against CIGAR ----

@pytest.mark.parametrize("case", m.NM_CASES, ids=lambda c: "e%d-L%d" % (c[1], c[2]))
def test_seq_agrees_with_nm_after_the_rule_and_not_before(case):
    c = m.nm_case(*case)
    off = m.expected(c)
    fwd, fwd_ok, rev, rev_ok = m.nm_agreement(off, c["seqs"], c["names"])
    assert fwd >= 100 and rev >= 100 and fwd_ok == fwd and rev_ok == 0
    fwd2, fwd_ok2, rev2, rev_ok2 = m.nm_agreement(m.apply(off), c["seqs"], c["names"])
    assert (fwd2, fwd_ok2, rev2) == (fwd, fwd, rev) and rev_ok2 == rev


# ---- what the generators reach, by the oracle ----

def test_the_ladder_has_every_length_on_both_strands():
    c = m.ladder_case()
    off = m.expected(c)
    assert sorted(set(len(r) for r in c["reads"])) == sorted(m.LADDER)
    seen = m.ladder_strands(off, c)
    assert all(seen.get(L) == {0, 16} for L in m.LADDER), seen
    assert len(m.turned(off)) == len(m.LADDER)
    strands = [m.flag_of(l) & 16 for l in off.splitlines()]
    lens = [len(l.split(b"\t")[9]) for l in off.splitlines()]
    pairs = list(zip(range(0, len(strands) - 1, 2), range(1, len(strands), 2)))  # the two records a wave renders together
    assert sum(strands[a] != strands[b] for a, b in pairs) >= 4 and all(lens[a] != lens[b] for a, b in pairs)
    q = "".join(c["quals"])
    assert min(q) == "!" and max(q) == "~"
    for L in m.LADDER:  # the packed staging takes one length at a time: both strands there, too
        keep = [i for i, r in enumerate(c["reads"]) if len(r) == L]
        assert len(keep) == 2


def test_the_letters_case_maps_its_odd_reads_on_the_reverse_strand():
    c = m.letters_case()
    res = c["res"]
    primary = {r: int(res.r_flag[int(res.rec_off[r])]) for r in range(len(c["reads"])) if res.rec_off[r + 1] > res.rec_off[r]}
    odd = [r for r, read in enumerate(c["reads"]) if any(ch in m.ODD_LETTERS for ch in read)]
    rev_odd = [r for r in odd if primary.get(r, 0) & 16]
    assert len(rev_odd) >= 20
    for ch in m.ODD_LETTERS:
        assert any(ch in c["reads"][r] for r in rev_odd), chr(ch)
    assert set(sum(ch in m.ODD_LETTERS for ch in c["reads"][r]) for r in rev_odd) == {1, 2, 3}
    lower = [r for r, read in enumerate(c["reads"]) if read != read.upper()]
    assert len(lower) == 2 and all(primary[r] & 16 for r in lower) and any(len(c["reads"][r]) % 2 for r in lower)
    assert any(f & 0x8000 and f & 16 for f in primary.values()) and any(f & 0x8000 and not f & 16 for f in primary.values())
    assert len(m.turned(m.expected(c))) >= 20


def test_the_pairs_case_has_rescued_mates_turned_and_lines_placed_at_reversed_mates():
    from tests import cases, report_model as rp, tags_model as tm
    c = cases.line_options_case()
    text, dropped = rp.paired(c["want"], c["n"], c["names"], c["reads"], c["rnames"], c["quals"], cases.I, cases.X, res=c["ext"],
                              rescued=set(c["kept"]), e=cases.LINE_E, strata=cases.STRATA, max_hits=cases.MAX_HITS)
    text = tm.apply(text, cases.RG, True)
    assert dropped > 0 and len(m.turned(text)) >= 20
    assert len(m.rescued_turned(text, c)) >= 3
    placed = m.placed_at_reversed(text)
    assert placed and all(l + b"\n" in m.apply(text) for l in placed)
    on = m.apply(text)
    assert len(on) == len(text) and [l.split(b"\t")[11:] for l in on.splitlines()] == [l.split(b"\t")[11:] for l in text.splitlines()]


def test_the_drawn_option_sets():
    from tests import cases
    assert len(m.DRAW_CASES) * m.DRAWS_PER_CASE >= 16
    sets = [tuple(sorted((k, str(v)) for k, v in d.items())) for k in range(len(m.DRAW_CASES)) for d in m.draws(k)]
    assert len(set(sets)) >= 16 and m.draws(0) == m.draws(0)  # fixed: the same draws every time
    assert all(hasattr(cases, maker) for _, maker, _ in m.DRAW_CASES)
    assert any(d["paired"] and d["rescue"] for d in m.draws(2) + m.draws(3)) and any(d["mate_tags"] and d["paired"] for d in m.draws(2) + m.draws(3))
    assert not any(d["paired"] for d in m.draws(0) + m.draws(1))


# ---- the command line ----

def test_usage_lists_the_switch():
    r = run_fem("map", "-h")
    assert r.returncode == 0 and b"--sam-seq" in r.stderr and b"SEQ reverse-complemented and QUAL reversed" in r.stderr


@pytest.mark.parametrize("extra", [(), ("--read2", "c2"), ("--bam",), ("--read2", "c2", "--mate-tags", "--bam=0", "-t", "24")])
def test_the_switch_is_accepted(extra):
    # (the next refusal is the reference file that is not there: the option itself passed)
    r = run_fem(*(BASE + ("--sam-seq",) + extra))
    first = r.stderr.splitlines()[0] if r.stderr else b""
    assert r.returncode != 0 and b"sam-seq" not in first and b"Usage" not in first and b"unrecognized" not in r.stderr


@pytest.mark.parametrize("var", ["FEM_HOST_TAIL", "FEM_HOST_FORMAT", "FEM_HOST_QUALS"])
def test_refused_with_host_text_or_host_qualities(var):
    r = run_fem(*(BASE + ("--sam-seq",)), env={var: "1"})
    assert r.returncode == 1 and (b"--sam-seq is not supported with %s=1" % var.encode()) in r.stderr
    assert b"Loaded index" not in r.stderr
    r = run_fem(*BASE, env={var: "1"})  # without the switch the variable is none of its business
    assert b"--sam-seq" not in r.stderr.split(b"Usage")[0]


# ---- the ABI ----

def test_the_symbol_is_in_the_header_the_binding_and_the_library():
    from fem_amd.device import ABI_SYMBOLS, Device, hip_library_path
    from tests.cases import declared_symbols
    assert "fem_dev_set_sam_seq" in set(ABI_SYMBOLS) & set(declared_symbols())
    assert callable(getattr(Device, "set_sam_seq"))
    lib = ctypes.CDLL(hip_library_path())
    assert hasattr(lib, "fem_dev_set_sam_seq")
    hdr = open(os.path.join(ROOT, "include", "fem_hip.h")).read()
    assert "int fem_dev_set_sam_seq(fem_dev *h, int slot, int on);" in hdr and "=ACMGRSVTWYHKDBN to =TGKCYSBAWRDMHVN" in hdr
    # the qualities-on-the-host path is refused at fetch time: the header says so and the library carries the message
    assert "fem_dev_commit_names_stage, where the caller fills the QUAL holes forward) is FEM_ERR_INVALID" in hdr
    assert b"(fem_dev_set_sam_seq) need the qualities on the device" in open(hip_library_path(), "rb").read()
