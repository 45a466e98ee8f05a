"""SEQ and QUAL as SAM orders them (fem_dev_set_sam_seq, FEM map --sam-seq), the rule in plain Python on SAM
text: apply() turns the text made without the option into the text made with it.  A line changes only if its FLAG has 0x10 and
it carries SEQ; then SEQ is reverse-complemented and QUAL reversed.  Also here, so that the CPU can check what they reach
(tests/test_sam_seq_model.py): the case generators of tests/test_gpu_sam_seq.py and the NM check that reads SEQ against CIGAR."""
import functools
import re

import numpy as np

from oracle import fem_oracle as fo
from tests import cases
from tests import util

LETTERS = "=ACMGRSVTWYHKDBN"      # what a SAM line prints: the letter of 4-bit code 0, 1, .. 15
COMPLEMENT = "=TGKCYSBAWRDMHVN"   # ... and the complement of each
_COMP = {ord(a): ord(b) for a, b in zip(LETTERS, COMPLEMENT)}


def printed(ch):
    """The letter a read character is printed as without the option (the 4-bit round trip): IUPAC upper-cased, else N."""
    up = chr(ch).upper()
    return ord(up) if up in LETTERS else ord("N")


def revcomp(seq):
    """The reverse complement of a SEQ field (bytes); a character that no line prints goes through printed() first."""
    return bytes(_COMP[printed(c)] for c in reversed(seq))


def flag_of(line):
    return int(line.split(b"\t", 2)[1])


def apply(text):
    """The SAM text (bytes; header lines allowed) with the option on, from the same text with the option off."""
    out = []
    for line in text.split(b"\n"):
        if line and not line.startswith(b"@"):
            f = line.split(b"\t")
            if int(f[1]) & 16 and f[9] != b"*":
                f[9] = revcomp(f[9])
                if f[10] != b"*":
                    f[10] = f[10][::-1]
                line = b"\t".join(f)
        out.append(line)
    return b"\n".join(out)


def turned(text):
    """The lines of a text that apply() changes: the reverse-strand lines that carry SEQ."""
    return [l for l in text.splitlines() if l and not l.startswith(b"@") and flag_of(l) & 16 and l.split(b"\t")[9] != b"*"]


# ---- SEQ read against CIGAR: mismatches plus inserted and deleted bases, which is what NM:i says ----

def nm_by_cigar(line, seqs, names):
    """Walks the line's CIGAR over its SEQ and the reference from POS -> mismatches + I lengths + D lengths (None: CIGAR *)."""
    f = line.split(b"\t")
    if f[5] == b"*":
        return None
    ref, p, i, n = seqs[names.index(f[2].decode())], int(f[3]) - 1, 0, 0
    seq = f[9]
    for ln, op in re.findall(rb"(\d+)([MID])", f[5]):
        ln = int(ln)
        if op == b"M":
            n += sum(1 for k in range(ln) if seq[i + k] != ref[p + k])
            i, p = i + ln, p + ln
        elif op == b"I":
            n, i = n + ln, i + ln
        else:
            n, p = n + ln, p + ln
    assert i == len(seq)
    return n


def nm_tag(line):
    return int(next(t for t in line.split(b"\t")[11:] if t.startswith(b"NM:i:"))[5:])


def nm_agreement(text, seqs, names):
    """-> (forward lines, those whose SEQ agrees with NM, reverse-strand lines, those that agree), over the lines with SEQ and CIGAR."""
    fwd = fwd_ok = rev = rev_ok = 0
    for l in text.splitlines():
        f = l.split(b"\t")
        if l.startswith(b"@") or f[9] == b"*" or f[5] == b"*":
            continue
        ok = nm_by_cigar(l, seqs, names) == nm_tag(l)
        if int(f[1]) & 16:
            rev, rev_ok = rev + 1, rev_ok + ok
        else:
            fwd, fwd_ok = fwd + 1, fwd_ok + ok
    return fwd, fwd_ok, rev, rev_ok


# seed, e, L, n reads, repeat-rich reference: upper-case ACGT reads without N
NM_CASES = [(601, 3, 100, 400, False), (602, 7, 150, 400, True), (603, 2, 65, 400, False), (604, 3, 129, 400, False)]


@functools.lru_cache(maxsize=None)
def nm_case(seed, e, L, n, repeats):
    rng = np.random.default_rng(seed)
    seqs, names = cases.reference(rng, repeats)
    reads = [r for r in util.make_reads(rng, seqs, 2 * n, L, e) if set(r) <= set(b"ACGT")][:n]  # (none across the reference's N runs)
    assert len(reads) == n
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    rnames = ["r%d" % i for i in range(n)]
    return dict(seqs=seqs, names=names, reads=reads, rnames=rnames, quals=rand_quals(rng, reads), e=e, ref=ref, idx=idx, res=res)


def expected(c):
    """The oracle's text of a case (option off), SEQ through the letter table (expected_sam only upper-cases)."""
    text = cases.expected_sam(c["names"], c["reads"], c["rnames"], c["quals"], c["res"]).encode("latin-1")
    out = []
    for l in text.splitlines():
        f = l.split(b"\t")
        f[9] = f[9] if f[9] == b"*" else bytes(printed(ch) for ch in f[9])
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def rand_quals(rng, reads):
    """Qualities drawn over '!'..'~'."""
    return [bytes(rng.integers(33, 127, len(r)).astype(np.uint8)).decode("latin-1") for r in reads]


# ---- the length ladder: every length on both strands, in one ragged batch at e = 0 ----

# one and two bytes per lane of sam_write_kernel and its tail loop (64, 128, 192, 256), odd and even, a BAM record's last
# nibble, the device's longest read
LADDER = (37, 63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 1023, 1024)


@functools.lru_cache(maxsize=None)
def ladder_case():
    """Each length of LADDER once as a forward copy and once as the reverse complement of a place of its own in a random
    reference, shuffled, so that the two records a wave of sam_write_kernel renders together mix strands and lengths."""
    rng = np.random.default_rng(611)
    seqs, names = [util.rand_seq(rng, 60_000)], ["ladder"]
    reads, at = [], 500
    for L in LADDER:
        reads.append(seqs[0][at:at + L])
        at += L + 300
        reads.append(util.revcomp(seqs[0][at:at + L]))
        at += L + 300
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=0, threads=4)
    return dict(seqs=seqs, names=names, reads=reads, rnames=["l%d" % i for i in range(len(reads))], quals=rand_quals(rng, reads), e=0,
                ref=ref, idx=idx, res=res)


def ladder_strands(text, c):
    """-> {length: set of the strands (0, 16) of its primary lines} of a text of the ladder."""
    seen = {}
    by_name = {n: len(r) for n, r in zip(c["rnames"], c["reads"])}
    for l in text.splitlines():
        f = l.split(b"\t")
        if f[9] != b"*":
            seen.setdefault(by_name[f[0].decode()], set()).add(int(f[1]) & 16)
    return seen


def sub_case(c, keep):
    """The case with the reads `keep` (indices) alone; the oracle's result is not carried over."""
    return dict(c, reads=[c["reads"][i] for i in keep], rnames=[c["rnames"][i] for i in keep], quals=[c["quals"][i] for i in keep], res=None)


# ---- letters: reverse-strand reads with IUPAC letters, '=' and '.', a lower-case read, a record with 0x8000 ----

ODD_LETTERS = b"NRYKM=."


@functools.lru_cache(maxsize=None)
def letters_case():
    """e = 3.  Sequence 0: random; sequence 1 has a lower-case stretch, on which an upper-case read is verified and not traced (FLAG
    0x8000, CIGAR *).  40 reverse-complemented reads with one to three of ODD_LETTERS (each costs an edit), one of them per
    letter at the least; a lower-case reverse-strand read; forward reads with such letters; reverse-strand reads on the lower-case stretch."""
    rng, L = np.random.default_rng(612), 100
    low = util.rand_seq(rng, 4000)
    seqs, names = [util.rand_seq(rng, 40_000), low[:1000] + low[1000:3000].lower() + low[3000:]], ["plain", "low"]
    reads = []
    for i in range(48):
        s0 = 300 + 700 * i
        r = bytearray(util.revcomp(seqs[0][s0:s0 + L]) if i < 40 else seqs[0][s0:s0 + L])
        for k in range(1 + i % 3):
            r[7 + 31 * k + i % 20] = ODD_LETTERS[(i + k) % len(ODD_LETTERS)]
        reads.append(bytes(r))
    reads.append(util.revcomp(seqs[0][35_000:35_000 + L]).lower())
    reads.append(util.revcomp(seqs[0][36_000:36_000 + L - 1]).lower().replace(b"a", b"A", 3))
    for s0 in (1200, 1500, 1800, 2100):  # upper-case reads on the lower-case stretch, both strands
        reads.append(util.revcomp(seqs[1][s0:s0 + L].upper()))
        reads.append(seqs[1][s0 + 150:s0 + 150 + L].upper())
    reads = [reads[i] for i in rng.permutation(len(reads))]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=3, threads=4)
    return dict(seqs=seqs, names=names, reads=reads, rnames=["x%d" % i for i in range(len(reads))], quals=rand_quals(rng, reads), e=3,
                ref=ref, idx=idx, res=res)


# ---- pairs: tests.cases.line_options_case() with every option on ----

def read_of_line(line, n):
    """The read (0 .. 2n - 1) of a line of a paired text whose names are p<i>."""
    f = line.split(b"\t", 2)
    return int(f[0][1:]) + (n if int(f[1]) & 0x80 else 0)


def rescued_turned(text, c):
    """The lines apply() changes that are rescued mates': their read has no single-end record (c: line_options_case())."""
    off = c["want"].rec_off
    return [l for l in turned(text) if off[read_of_line(l, c["n"]) + 1] == off[read_of_line(l, c["n"])]]


def placed_at_reversed(text):
    """The lines of unmapped reads placed at a reversed mate: 0x4 and 0x20, and never 0x10."""
    return [l for l in text.splitlines() if flag_of(l) & 4 and flag_of(l) & 0x20]


# ---- drawn option sets over tests.cases' cases ----

DRAW_CASES = [("single", "unmapped_single_case", cases.UNMAPPED_SINGLE_CASES[0]), ("single-repeats", "report_single_case", cases.REPORT_SINGLE_CASES[0]),
              ("pairs-rescue", "unmapped_pair_case", cases.UNMAPPED_PAIR_CASES[2]), ("pairs-repeats", "report_pair_case", cases.REPORT_PAIR_CASES[0])]
DRAWS_PER_CASE = 5


def draws(k):
    """The option sets drawn for DRAW_CASES[k]: a subset of the line options each; pair mode only for a case of pairs.  They are
    compared with the device's own text with the option off, which the line fuzzer (tests/fuzz_lines.py) now ties to the oracle
    under drawn options."""
    rng = np.random.default_rng(620 + k)
    paired_case = DRAW_CASES[k][1].endswith("pair_case")
    out = []
    for _ in range(DRAWS_PER_CASE):
        coin = lambda: bool(rng.random() < 0.5)  # noqa: E731
        d = dict(paired=paired_case and rng.random() < 0.8, mapq=coin(), unmapped=coin(), strata=[None, 0, 1][int(rng.integers(0, 3))],
                 max_hits=[None, 1, 3][int(rng.integers(0, 3))], rg=b"grp.1" if coin() else None, hits=coin())
        d.update(rescue=d["paired"] and coin(), discordant=coin(), mate_tags=coin(), orientation=int(rng.integers(0, 3)) if coin() else 0)
        out.append(d)
    return out
