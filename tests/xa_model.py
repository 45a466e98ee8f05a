"""The rule of fem_dev_set_xa / FEM map --xa in plain Python, on SAM text without header lines (include/fem_hip.h and DESIGN.md
§4.6m state it in words): a slot's secondary lines folded into an XA:Z field on its primary line.

A line without FLAG 0x100 opens a slot; the following lines with 0x100 are its secondary lines l_1 .. l_{c-1}.  The entry of l_t is
<RNAME>,<s><POS>,<CIGAR>,<NM>; with the bytes of those columns as the line prints them, s = - where its FLAG has 0x10, else +, and
the digits of its NM:i.  f is the largest f <= min(c - 1, N) whose entries 1 .. f have at most MAX_BYTES bytes together; with f >= 1
the lines l_1 .. l_f go and l_0 gains one last field, XA:Z: and those entries; every other byte stays.

Also here, as tests/sam_seq_model.py keeps them: the cases and the drawn option sets of tests/test_gpu_xa.py."""
import functools

import numpy as np

from oracle import fem_oracle as fo
from tests import cases
from tests import util

MAX_BYTES = 8192     # FEM_XA_MAX_BYTES
ALL = 2 ** 31 - 1    # no entry limit: the byte budget alone bounds a slot's folding


def flag_of(line):
    return int(line.split(b"\t", 2)[1])


def entry(line):
    """The XA entry a secondary line folds into."""
    f = line.split(b"\t")
    nm = [x for x in f[11:] if x.startswith(b"NM:i:")]
    assert len(nm) == 1, line
    return b"%s,%s%s,%s,%s;" % (f[2], b"-" if int(f[1]) & 16 else b"+", f[3], f[5], nm[0][5:])


def slots(text):
    """The lines of a text grouped by slot: a line without 0x100 and the lines with 0x100 behind it."""
    out = []
    for l in text.splitlines():
        if flag_of(l) & 0x100:
            assert out, "a secondary line in front of every primary one"
            out[-1].append(l)
        else:
            out.append([l])
    return out


def folded(slot, max_entries, max_bytes=MAX_BYTES):
    """f of a slot's lines."""
    f = total = 0
    for l in slot[1:]:
        n = len(entry(l))
        if f >= max_entries or total + n > max_bytes:
            break
        f, total = f + 1, total + n
    return f


def apply(text, max_entries, max_bytes=MAX_BYTES):
    """-> (the text with the option on at N = max_entries, the number of entries)."""
    out, n_entries = [], 0
    for slot in slots(text):
        f = folded(slot, max_entries, max_bytes)
        n_entries += f
        out.append(slot[0] + (b"\tXA:Z:" + b"".join(entry(l) for l in slot[1:1 + f]) if f else b""))
        out += slot[1 + f:]
    return b"".join(l + b"\n" for l in out), n_entries


def xa_of(line):
    """The value of a line's XA:Z field, None without one; the field is the line's last."""
    f = line.split(b"\t")[11:]
    at = [i for i, x in enumerate(f) if x.startswith(b"XA:Z:")]
    assert at in ([], [len(f) - 1]), line
    return f[-1][5:] if at else None


def entries(line):
    """The entries of a line's XA value as (RNAME, strand, POS, CIGAR, NM) tuples of bytes; [] without the field."""
    v = xa_of(line)
    if v is None:
        return []
    assert v.endswith(b";")
    out = []
    for e in v[:-1].split(b";"):
        rname, pos, cigar, nm = e.rsplit(b",", 3)  # (an RNAME may hold commas; the other three cannot)
        assert pos[:1] in (b"+", b"-") and pos[1:].isdigit() and nm.isdigit(), e
        out.append((rname, pos[:1], pos[1:], cigar, nm))
    return out


def unfold(text_on):
    """Per folded entry, in order, the (QNAME, strand, RNAME, POS, CIGAR, NM) it stands for."""
    out = []
    for l in text_on.splitlines():
        q = l.split(b"\t", 1)[0]
        out += [(q, s, rname, pos, cigar, nm) for rname, s, pos, cigar, nm in entries(l)]
    return out


def columns(line):
    """What unfold gives back of a secondary line."""
    f = line.split(b"\t")
    nm = [x for x in f[11:] if x.startswith(b"NM:i:")][0][5:]
    return (f[0], b"-" if int(f[1]) & 16 else b"+", f[2], f[3], f[5], nm)


def tag(line, name):
    """The value of tag `name` (b"NH:i") on a line, None without it."""
    for x in line.split(b"\t")[11:]:
        if x.startswith(name + b":"):
            return x[len(name) + 1:]
    return None


def budget_stops(text, max_entries=ALL):
    """The slots of a text (option off) whose folding stops for the byte budget: (lines, f) with f < min(c - 1, N)."""
    out = []
    for slot in slots(text):
        f = folded(slot, max_entries)
        if f < min(len(slot) - 1, max_entries):
            out.append((slot, f))
    return out


# ---- cases of tests/test_gpu_xa.py ----

N_LADDER = (1, 2, 31, 32, 33, 63, 64, 65, ALL)   # a lane's slot and its last line, the wave's first, one step, two, many
FOLD_SIZES = (1, 31, 32, 63, 64)                 # c - 1 of the slots that must occur (and one of 199 entries or more)


def long_names(c, exact=60, rich=200):
    """The case with long reference names: `exact` characters for the sequence with the units in k copies (chr3), `rich` for the
    first repeat-rich one (chr0); the records are the same, so the oracle's result stays."""
    names = list(c["names"])
    names[3] = "exact_" + "e" * (exact - 6)
    names[0] = "rich_" + "r" * (rich - 5)
    return dict(c, names=names)


@functools.lru_cache(maxsize=None)
def star_case():
    """e = 3.  One unit of 160 bases in three copies with flanks of their own, the first in upper case and the other two in lower
    case, and upper-case reads over it: the copies in lower case verify and are not traced (FLAG 0x8000, CIGAR *), as
    sam_seq_model.letters_case gets such records, here as SECONDARY records of slots whose primary is the upper-case copy.  Reads on
    both strands; a random sequence with plain reads beside it."""
    rng, L = np.random.default_rng(641), 100
    unit = util.rand_seq(rng, 160)
    parts = [util.rand_seq(rng, 500), unit, util.rand_seq(rng, 700), unit.lower(), util.rand_seq(rng, 900), unit.lower(), util.rand_seq(rng, 400)]
    seqs, names = [util.rand_seq(rng, 30_000), b"".join(parts)], ["plain", "units"]
    reads = []
    for o in (0, 7, 19, 33, 48, 60):
        reads.append(unit[o:o + L])
        reads.append(util.revcomp(unit[o:o + L]))
    reads += util.make_reads(rng, seqs[:1], 20, L, 2)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=3, threads=4)
    return dict(seqs=seqs, names=names, reads=reads, rnames=["s%d" % i for i in range(len(reads))], quals=cases.quals(reads), e=3,
                ref=ref, idx=idx, res=res)


def star_secondaries(c):
    """The secondary records of star_case with 0x8000, from the oracle: (read, record) pairs."""
    res, out = c["res"], []
    for r in range(len(c["reads"])):
        lo, hi = int(res.rec_off[r]), int(res.rec_off[r + 1])
        out += [(r, j) for j in range(lo + 1, hi) if int(res.r_flag[j]) & 0x8000]
    return out


@functools.lru_cache(maxsize=None)
def equal_length_case():
    """Reads of one length without N on a repeat-rich reference: the batch the 2-bit staging takes."""
    rng = np.random.default_rng(642)
    seqs, names = cases.reference(rng, True)
    reads = [r for r in util.make_reads(rng, seqs, 600, 100, 3) if set(r) <= set(b"ACGT")][:300]
    assert len(reads) == 300
    return dict(seqs=seqs, names=names, reads=reads, rnames=["q%d" % i for i in range(len(reads))], quals=cases.quals(reads), e=3, idx=None)


# ---- drawn option sets over tests.cases' cases (each on a repeat-rich reference: without secondary lines nothing folds) ----

DRAW_CASES = [("single", "unmapped_single_case", cases.UNMAPPED_SINGLE_CASES[1]), ("single-repeats", "report_single_case", cases.REPORT_SINGLE_CASES[0]),
              ("pairs-rescue", "unmapped_pair_case", cases.UNMAPPED_PAIR_CASES[1]), ("pairs-repeats", "report_pair_case", cases.REPORT_PAIR_CASES[0])]
DRAWS_PER_CASE = 5


def draws(k):
    """The option sets drawn for DRAW_CASES[k]: a subset of the line options each with an entry limit of its own; pair mode only
    for a case of pairs.  They are compared with the device's own text with the option off, which the line fuzzer
    (tests/fuzz_lines.py) now ties to the oracle under drawn options."""
    rng = np.random.default_rng(650 + k)
    paired_case = DRAW_CASES[k][1].endswith("pair_case")
    out = []
    for _ in range(DRAWS_PER_CASE):
        coin = lambda: bool(rng.random() < 0.5)  # noqa: E731
        d = dict(paired=paired_case and rng.random() < 0.8, mapq=coin(), unmapped=coin(), strata=[None, 0, 1][int(rng.integers(0, 3))],
                 max_hits=[None, 1, 3, 40][int(rng.integers(0, 4))], rg=b"grp.1" if coin() else None, hits=coin(), sam_seq=coin())
        d.update(rescue=d["paired"] and coin(), discordant=coin(), mate_tags=coin(), orientation=int(rng.integers(0, 3)) if coin() else 0)
        d["xa"] = [1, 3, ALL][int(rng.integers(0, 3))]
        out.append(d)
    return out
