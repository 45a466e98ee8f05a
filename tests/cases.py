"""Inputs and expected values that more than one test module needs, all made on the CPU: references, reads, read pairs,
qualities, FASTA / FASTQ files, the expected SAM text of the oracle's records, the case generators of the output-line options
and the independent alignment models.  Nothing here opens a device or runs the FEM binary (that is tests/harness.py), and no
test module imports another: what two of them share lives here or there.  The case generators of the --unmapped, --strata /
--max-hits and tag tests are also run without a GPU (tests/test_unmapped_model.py, test_report_model.py, test_tags_model.py):
they must give the lines, slot sizes and hit counts those tests ask for."""
import functools
import gzip
import hashlib
import os
import re
import struct

import numpy as np

from oracle import fem_oracle as fo
from tests import discordant_fixture as df
from tests import discordant_model as dm
from tests import pair_model as pm
from tests import rescue_model as rm
from tests import unmapped_model as um
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, X = 0, 500  # the insert size range of the paired cases below


# ---- references, qualities, files ----

def reference(rng, repeats, second=60_000, name_pad=None):
    """Three repeat-rich sequences and a random one of 120 000 bases, or random sequences of 200 000 and `second` bases.
    -> seqs, names: chr0, chr1, ..; with name_pad, chr<i>_ followed by i * name_pad letters."""
    if repeats:
        seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200)
        seqs.append(util.rand_seq(rng, 120_000))
    else:
        seqs = [util.rand_seq(rng, 200_000), util.rand_seq(rng, second)]
    if name_pad is None:
        return seqs, ["chr%d" % i for i in range(len(seqs))]
    return seqs, ["chr%d_%s" % (i, "x" * (i * name_pad)) for i in range(len(seqs))]


def quals(reads):
    return ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]


def write_fastq(path, reads, names, quals, gz):
    import gzip
    data = "".join("@%s comment\n%s\n+\n%s\n" % (n, r.decode("latin-1"), q) for n, r, q in zip(names, reads, quals)).encode("latin-1")
    if gz:
        with gzip.open(str(path), "wb") as f:
            f.write(data)
    else:
        path.write_bytes(data)


def write_case(tmp_path, seed, e, L, n_reads, gz):
    rng = np.random.default_rng(seed)
    seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=40, spacer=200)
    seqs.append(util.rand_seq(rng, 150_000))
    names = ["chr%s" % c for c in "ABCD"]
    reads = util.make_reads(rng, seqs, n_reads, L, e, n_rate=0.002)
    rnames = ["read_%d" % i for i in range(n_reads)]
    quals = ["".join(chr(33 + (7 * i + j) % 41) for j in range(L)) for i in range(n_reads)]
    fa = tmp_path / "ref.fa"
    with open(fa, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b" some description\n")
            for i in range(0, len(s), 70):
                f.write(s[i:i + 70] + b"\n")
    fq = tmp_path / ("reads.fq.gz" if gz else "reads.fq")
    op = gzip.open if gz else open
    with op(fq, "wb") as f:
        for n, r, q in zip(rnames, reads, quals):
            f.write(b"@" + n.encode() + b" 1:N:0\n" + r + b"\n+\n" + q.encode() + b"\n")
    return seqs, names, reads, rnames, quals, str(fa), str(fq)


def expected_sam(seqs_names, reads, names, quals, res):
    """SAM v1 text for the oracle's records (field rules of src/align.c:546-632, src/map.c:50-55)."""
    lines = []
    for r in range(len(reads)):
        lo, hi = int(res.rec_off[r]), int(res.rec_off[r + 1])
        for j in range(lo, hi):
            primary = j == lo
            lines.append("\t".join([
                names[r], str(int(res.r_flag[j])), seqs_names[int(res.r_tid[j])], str(int(res.r_pos[j]) + 1), "255",
                res.cigar_str(j), "*", "0", "0",
                reads[r].decode().upper() if primary else "*", quals[r] if primary else "*",
                "NM:i:%d" % int(res.r_nm[j]), "MD:Z:" + res.md_str(j)]))
    return "".join(l + "\n" for l in lines)


def bgzf(data, block=65280, level=1, eof_block=True):
    """bgzip's format (SAM specification 4.1): gzip members with the 'BC' extra subfield, one per <= 64 KiB of input."""
    import struct
    import zlib
    out = []
    for at in list(range(0, len(data), block)) + ([None] if eof_block else []):
        chunk = b"" if at is None else data[at:at + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = c.compress(chunk) + c.flush()
        bsize = 18 + len(payload) + 8
        out.append(b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
                   + payload + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    return b"".join(out)


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "fem_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fem_[a-z0-9_]+)\s*\(", text)))


# ---- read pairs ----

def make_pairs(rng, seqs, n, L, e, L2=None):
    """n read pairs from fragments of 150-600 bp: mate 1 the fragment's first L bases, mate 2 the reverse complement of its last
    L2, 0..e edits each, mates swapped half the time; ~10 % discordant (other sequence, too far apart, same strand), ~10 % with
    one random mate, a few with both random."""
    L2 = L2 or L
    lens = np.array([len(s) for s in seqs], np.int64)
    ok = np.nonzero(lens > 700)[0]
    r1, r2 = [], []

    def mut(s, ln):
        s = util.mutate(rng, s, int(rng.integers(0, e + 1)))[:ln]
        return s + util.rand_seq(rng, ln - len(s)) if len(s) < ln else s

    for i in range(n):
        si = int(ok[rng.integers(0, len(ok))])
        frag = int(rng.integers(max(150, L, L2), 601))
        st = int(rng.integers(0, lens[si] - frag - e - 1))
        f = seqs[si][st:st + frag + e]
        a = mut(f[:L + e], L)
        b = mut(util.revcomp(f[frag - L2:frag + e][:L2 + e]), L2)
        kind = rng.random()
        if kind < 0.03:
            other = int(ok[rng.integers(0, len(ok))])
            so = int(rng.integers(0, lens[other] - L2 - e - 1))
            b = mut(util.revcomp(seqs[other][so:so + L2 + e]), L2)  # another sequence (or far away on the same one)
        elif kind < 0.06:
            far = min(int(lens[si]) - L2 - e - 1, st + 5000)
            if far > st + 700:
                b = mut(util.revcomp(seqs[si][far:far + L2 + e]), L2)  # too far apart
        elif kind < 0.10:
            b = mut(f[frag - L2:frag + e], L2)  # same strand
        elif kind < 0.15:
            a = util.rand_seq(rng, L)  # one random mate
        elif kind < 0.20:
            b = util.rand_seq(rng, L2)
        elif kind < 0.22:
            a, b = util.rand_seq(rng, L), util.rand_seq(rng, L2)
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    return r1, r2


def make_rescue_pairs(rng, seqs, n, L, L2, e, E, X, frac=0.4, near_end=False):
    """n read pairs from fragments of max(L, L2)..X bp (mate 1 forward, mate 2 the reverse complement of the fragment's end,
    mates swapped half the time).  0..e edits per mate; in `frac` of the pairs one mate carries e + 1 .. E edits instead
    (substitutions and indels), which single-end mapping at e misses.  near_end: some fragments at a sequence's ends."""
    lens = np.array([len(s) for s in seqs], np.int64)
    ok = np.nonzero(lens > X + 200)[0]
    r1, r2 = [], []

    def fit(s, ln):
        return s[:ln] if len(s) >= ln else s + util.rand_seq(rng, ln - len(s))

    for i in range(n):
        si = int(ok[rng.integers(0, len(ok))])
        frag = int(rng.integers(max(L, L2) + 20, X + 1))
        if near_end and i % 5 == 0:
            st = int(rng.integers(0, 3)) if i % 10 == 0 else int(lens[si]) - frag - int(rng.integers(0, 3))
        else:
            st = int(rng.integers(0, lens[si] - frag))
        f = seqs[si][st:st + frag]
        a, b = f[:L], util.revcomp(f[frag - L2:])
        heavy = rng.random() < frac
        ka = int(rng.integers(0, e + 1))
        kb = int(rng.integers(e + 1, E + 1)) if heavy and E > e else int(rng.integers(0, e + 1))
        a, b = fit(util.mutate(rng, a, ka), L), fit(util.mutate(rng, b, kb), L2)
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    return r1, r2


# ---- the single-end case of the SAM and BAM tests ----

def sam_case(seed, e, L, n_reads, repeats, odd):
    rng = np.random.default_rng(seed)
    long_fields = L > 200  # names, reference names and MD strings beyond one and two bytes per lane of sam_write_kernel
    seqs, names = reference(rng, repeats, 50_000, 70 if long_fields else 7)
    reads = util.make_reads(rng, seqs, n_reads, L, e, n_rate=0.003)
    if odd:
        reads[3] = reads[3].lower()
        reads[5] = reads[5][:L // 2] + b"RYKM=.-*"[:min(8, L - L // 2)] + reads[5][L // 2 + 8:]
        reads[7] = reads[7][:L - 17]  # a different length
    rnames = ["read_%d/%s" % (i, "n" * (i % (150 if long_fields else 40))) for i in range(len(reads))]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    return ref, idx, seqs, names, reads, rnames, quals(reads)


# ---- the cases of --unmapped: unmapped reads by construction (reads of random letters, reads with more than e edits) ----

# seed, e, L, n, repeat-rich reference, odd reads (lengths, letters, N runs, a read of length 0)
UNMAPPED_SINGLE_CASES = [(101, 3, 100, 1500, False, True), (102, 3, 100, 1200, True, False), (103, 7, 150, 600, True, True),
                         (104, 0, 64, 800, False, False)]


def unmapped_single_case(seed, e, L, n, repeats, odd):
    rng = np.random.default_rng(seed)
    seqs, names = reference(rng, repeats)
    reads = util.make_reads(rng, seqs, n, L, e, n_rate=0.002)
    for i in range(n):
        u = rng.random()
        if u < 0.2:
            reads[i] = util.rand_seq(rng, L)  # random letters
        elif u < 0.3:
            reads[i] = util.mutate(rng, util.make_reads(rng, seqs, 1, L + 10, 0)[0], e + 4)[:L]  # more than e edits
    if odd:
        reads[3] = reads[3].lower()
        reads[5] = reads[5][:L // 2] + b"RYKM=.-*" + reads[5][L // 2 + 8:]
        reads[7] = reads[7][:L - 17]
        reads[8] = util.rand_seq(rng, L - 31).lower()
        reads[9] = reads[9][:20] + b"N" * 40 + reads[9][60:]
        reads[10] = util.rand_seq(rng, 30) + b"n" * (L - 50) + util.rand_seq(rng, 20)
        reads[11] = b""
        reads[12] = util.rand_seq(rng, L + 60)
    rnames = ["read_%d_%s" % (i, "n" * (130 if i % 3 == 0 else i % 20)) for i in range(n)]  # names over 128 characters
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    return dict(seqs=seqs, names=names, reads=reads, rnames=rnames, quals=quals(reads), e=e, ref=ref, idx=idx, res=res,
                repeats=repeats, odd=odd)


def check_unmapped_single_case(c):
    n = len(c["reads"])
    counts = np.diff(c["res"].rec_off.astype(np.int64))
    n_unm = int(np.count_nonzero(counts == 0))
    assert 0.05 * n <= n_unm <= 0.95 * n, (n_unm, n)
    if c["repeats"]:  # reads with tens of records next to unmapped ones
        assert any(counts[r] >= 20 and (counts[r - 1] == 0 or counts[r + 1] == 0) for r in range(1, n - 1))
    if c["odd"]:
        assert counts[11] == 0 and len(c["reads"][11]) == 0
        assert any(counts[r] == 0 and len(c["rnames"][r]) > 128 for r in range(n))
        assert len(set(len(r) for r in c["reads"])) > 3


# seed, e, L, n pairs, repeat-rich reference, E of mate rescue (None: off)
UNMAPPED_PAIR_CASES = [(111, 3, 100, 900, False, None), (112, 3, 100, 700, True, None), (113, 2, 100, 700, False, 8),
                       (114, 2, 100, 600, True, 8)]


def unmapped_pair_case(seed, e, L, n, repeats, E):
    rng = np.random.default_rng(seed)
    seqs, names = reference(rng, repeats)
    if E is None:
        r1, r2 = make_pairs(rng, seqs, n, L, e)
    else:  # a mate with e + 1 .. E edits in a quarter of the pairs: lost by the mapping, found by the rescue
        r1, r2 = make_rescue_pairs(rng, seqs, n, L, L, e, E, X, frac=0.25)
    for i in range(n):  # mates of random letters: lost for good
        u = rng.random()
        if u < 0.12 or u >= 0.9:
            r1[i] = util.rand_seq(rng, L)
        if u >= 0.8:
            r2[i] = util.rand_seq(rng, L)
    r1[4], r2[6] = b"", r2[6].lower()
    r1[5] = util.rand_seq(rng, L - 13)
    reads = r1 + r2
    base = ["p%d_%s" % (i, "n" * (i % 140)) for i in range(n)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    withr, kept = None, {}
    if E is not None:
        withr, kept, _ = rm.rescue(res, n, reads, seqs, E, I, X)
    return dict(seqs=seqs, names=names, reads=reads, rnames=base + base, quals=quals(reads), e=e, E=E, n=n, ref=ref, idx=idx,
                res=res, withr=withr, kept=kept)


def check_unmapped_pair_case(c):
    n, after = c["n"], c["withr"] if c["withr"] is not None else c["res"]
    assert min(um.pair_classes(c["res"], n)) >= 20, um.pair_classes(c["res"], n)
    n_unm = len(um.unmapped_reads(after, 2 * n))
    assert 0.05 * 2 * n <= n_unm <= 0.95 * 2 * n
    if c["E"] is not None:
        assert len(c["kept"]) >= 20 and min(um.pair_classes(after, n)) >= 20
        lost = [r for r in um.unmapped_reads(after, 2 * n) if int(after.rec_off[(r + n) % (2 * n) + 1]) > int(after.rec_off[(r + n) % (2 * n)])]
        assert len(lost) >= 20  # mates that stay unmapped beside a mapped one


# ---- the cases of --strata / --max-hits: slots of every size at which the kernels take another path ----

# the slot sizes every case must hold: none, one, two, a lane's last (32), the wave's first (33), one step (64), two (65), many
SIZES = (0, 1, 2, 32, 33, 64, 65)
COPIES = (2, 32, 33, 64, 65, 210)


def report_reference(rng, L, copies=COPIES):
    """Sequences: two repeat-rich ones (diverged copies: slots whose lines span several NM), a random one (one line), `exact`
    (for every k of `copies` a unit of its own in exactly k copies, each followed by a spacer of its own: k lines) and `loci`
    (one consensus unit at 12 loci, two clean and ten with 1 or 2 substitutions in the window [50, 50 + L), each followed by a
    flank of its own).  -> seqs, names, units [(unit, [offset of each copy in exact])], consensus, [(offset in loci, d)]."""
    rich = util.repeat_rich_reference(rng, n_seq=2, unit_len=300, n_units=4, copies=40, spacer=200)
    back = util.rand_seq(rng, 100_000)
    parts, n, units = [util.rand_seq(rng, 200)], 200, []
    for k in copies:
        u, at = util.rand_seq(rng, L + 60), []
        for _ in range(k):
            at.append(n)
            parts += [u, util.rand_seq(rng, L + 20)]
            n += 2 * L + 80
        units.append((u, at))
    cons = util.rand_seq(rng, 300)
    lparts, n, loci = [util.rand_seq(rng, 100)], 100, []
    for i in range(12):
        d = 0 if i < 2 else 1 + i % 2
        u = bytearray(cons)
        for pos in rng.choice(np.arange(60, 40 + L), d, replace=False):
            u[pos] = b"ACGT".replace(bytes([u[pos]]), b"")[int(rng.integers(0, 3))]
        loci.append((n, d))
        lparts += [bytes(u), util.rand_seq(rng, 300)]
        n += 600
    seqs = rich + [back, b"".join(parts), b"".join(lparts)]
    return seqs, ["chr%d" % i for i in range(len(seqs))], units, cons, loci


def _shuffled(rng, *lists):
    order = rng.permutation(len(lists[0]))
    return [[l[i] for i in order] for l in lists]


# seed, e, L, n
REPORT_SINGLE_CASES = [(201, 3, 100, 1200), (202, 7, 150, 600)]


@functools.lru_cache(maxsize=None)
def report_single_case(seed, e, L, n):
    rng = np.random.default_rng(seed)
    seqs, names, units, cons, loci = report_reference(rng, L)
    reads = util.make_reads(rng, seqs[:2], n // 2, L, min(e, 3), n_rate=0.002)
    reads += util.make_reads(rng, seqs[2:3], n // 4, L, e)
    for u, _ in units:  # 6 reads per unit, as they stand in it
        reads += [u[o:o + L] for o in rng.integers(0, 61, 6)]
    reads += [cons[50:50 + L]] * 6
    reads += [util.rand_seq(rng, L) for _ in range(n - len(reads))]
    reads, = _shuffled(rng, reads)
    rnames = ["read_%d_%s" % (i, "n" * (i % 20)) for i in range(n)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    return dict(seqs=seqs, names=names, reads=reads, rnames=rnames, quals=quals(reads), e=e, ref=ref, idx=idx, res=res)


def _slot_nms(res, r):
    return res.r_nm[int(res.rec_off[r]):int(res.rec_off[r + 1])]


def check_slots(res, n_reads):
    """Slots of every size in SIZES and of 200 lines or more; 20 slots or more whose lines span three NM values or more."""
    counts = np.diff(res.rec_off.astype(np.int64))[:n_reads]
    for k in SIZES:
        assert np.count_nonzero(counts == k) >= 1, (k, sorted(set(counts.tolist())))
    assert np.count_nonzero(counts >= 200) >= 1, sorted(set(counts.tolist()))
    assert sum(1 for r in range(n_reads) if len(set(_slot_nms(res, r).tolist())) >= 3) >= 20


def check_report_single_case(c):
    check_slots(c["res"], len(c["reads"]))


# seed, e, L, n pairs, E of mate rescue (None: off)
REPORT_PAIR_CASES = [(211, 3, 100, 700, None), (212, 2, 100, 700, 8)]


@functools.lru_cache(maxsize=None)
def report_pair_case(seed, e, L, n, E):
    rng = np.random.default_rng(seed)
    seqs, names, units, cons, loci = report_reference(rng, L)
    exact, lseq = seqs[3], seqs[4]
    r1, r2 = [], []
    for u, at in units:  # mate 1 in the unit (all its copies), mate 2 in the spacer behind one copy (4 pairs) or nowhere near (2)
        for t in range(6):
            o = int(rng.integers(0, 61))
            sp = at[int(rng.integers(0, len(at)))] + len(u)
            r1.append(u[o:o + L])
            r2.append(util.revcomp(exact[sp + 5:sp + 5 + L]) if t < 4 else util.make_reads(rng, seqs[2:3], 1, L, 0)[0])
    for at, d in loci:  # mate 1 the consensus (NM 0 at the clean loci, d here), mate 2 in this locus' flank: chosen here
        if d:
            r1.append(cons[50:50 + L])
            r2.append(util.revcomp(lseq[at + 350:at + 350 + L]))
    k = n - len(r1)
    if E is None:
        a, b = make_pairs(rng, seqs[:3], k, L, e)
    else:  # a mate with e + 1 .. E edits in a quarter of the pairs: lost by the mapping, found by the rescue
        a, b = make_rescue_pairs(rng, seqs[:3], k, L, L, e, E, X, frac=0.25)
        for i in range(k):  # mates of random letters: lost for good
            if rng.random() < 0.1:
                a[i] = util.rand_seq(rng, L)
    r1, r2 = r1 + a, r2 + b
    for i in range(0, len(r1), 2):  # (the mates swapped in half the pairs)
        r1[i], r2[i] = r2[i], r1[i]
    r1, r2 = _shuffled(rng, r1, r2)
    reads = r1 + r2
    base = ["p%d_%s" % (i, "n" * (i % 30)) for i in range(n)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    withr, kept = None, {}
    if E is not None:
        withr, kept, _ = rm.rescue(res, n, reads, seqs, E, I, X)
    return dict(seqs=seqs, names=names, reads=reads, rnames=base + base, quals=quals(reads), e=e, E=E, n=n, ref=ref, idx=idx,
                res=res, withr=withr, kept=kept)


def off_stratum_pairs(res, n_pairs):
    """Proper pairs in which a mate's chosen record has an NM above that mate's least."""
    found = 0
    for i, c in enumerate(pm.choose(res, n_pairs, I, X)):
        if c is not None:
            a, b = _slot_nms(res, i), _slot_nms(res, n_pairs + i)
            found += int(a[c[0]]) > int(a.min()) or int(b[c[1]]) > int(b.min())
    return found


def check_report_pair_case(c):
    after = c["withr"] if c["withr"] is not None else c["res"]
    check_slots(after, 2 * c["n"])
    assert off_stratum_pairs(after, c["n"]) >= 5
    if c["E"] is not None:
        assert len(c["kept"]) >= 20


# expected texts of those cases without the filter (made once per case and switch)

@functools.lru_cache(maxsize=None)
def _want_single(case, mapq):
    c = report_single_case(*case)
    return um.single_end(c["res"], c["names"], c["reads"], c["rnames"], c["quals"], e=c["e"] if mapq else None)


@functools.lru_cache(maxsize=None)
def _want_paired(case, mapq):
    c = report_pair_case(*case)
    return um.paired(c["res"], c["n"], c["names"], c["reads"], c["rnames"], c["quals"], I, X, res=c["withr"], rescued=set(c["kept"]),
                     e=c["e"] if mapq else None)


def report_want(case, paired, mapq, unmapped):
    text = (_want_paired if paired else _want_single)(case, mapq)
    return text if unmapped else um.without_unmapped(text, paired)[0]


# ---- hit counts of the NH / HI tags: slots of 130 lines among slots of 1 and 2 ----

@functools.lru_cache(maxsize=None)
def hits_case():
    rng = np.random.default_rng(310)
    L = 100
    seqs, names, units, _, _ = report_reference(rng, L, copies=(130, 2))
    seqs, names = seqs[2:4], names[2:4]  # the random sequence and the one with the units
    (u130, _), (u2, _) = units
    reads = [u130[o:o + L] for o in rng.integers(0, 61, 5)] + [u2[o:o + L] for o in rng.integers(0, 61, 4)]
    reads += util.make_reads(rng, seqs[:1], 7, L, 0)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=3, threads=4)
    return dict(seqs=seqs, names=names, reads=reads, rnames=["h%d" % i for i in range(len(reads))], quals=quals(reads), e=3, idx=idx,
                res=res)


# ---- every output-line option on one small batch of pairs (tests/test_gpu_line_options.py, test_gpu_mate_tags.py) ----

K_PAIR_ALONE = 32  # fem_tail.hip: pairs with more combinations are their wave's
LINE_E, LINE_RESCUE_E, LINE_L = 2, 8, 100
STRATA, MAX_HITS, RG = 1, 3, b"grp1"


@functools.lru_cache(maxsize=None)
def line_options_case():
    """46 pairs on a repeat-rich reference: discordant pairs, pairs with one heavy mate, plain ones, two that keep a mate
    (both mates) without a record; the oracle's single-end records and the models' results."""
    e, E, L = LINE_E, LINE_RESCUE_E, LINE_L
    rng = np.random.default_rng(7)
    main = [util.rand_seq(rng, 60_000)] + util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200)
    seqs, r1, r2 = df.make_discordant_pairs(rng, main, 44, L, L, e, E, X, n_sym=4, decoy_copies=2)
    r1 += [r1[2], util.rand_seq(rng, L)]
    r2 += [util.rand_seq(rng, L), util.rand_seq(rng, L)]
    n, reads = len(r1), r1 + r2
    names = ["chr%d" % i for i in range(len(seqs))]
    rnames = ["p%d" % i for i in range(n)] * 2
    quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    ext, kept, _, kinds = dm.rescue(want, n, reads, seqs, E, I, X)
    c = dict(seqs=seqs, names=names, reads=reads, rnames=rnames, quals=quals, idx=idx, want=want, ext=ext, kept=kept, n=n)
    c["n_kind2"] = sum(k == 2 for k, _ in kinds.values())
    c["n_proper"] = pm.expected(ext, n, I, X)[1]
    c["n_unmapped"] = len(um.unmapped_reads(ext, 2 * n))
    # the fixture does its job: both kinds of rescue, reads that stay unmapped, proper pairs, a pair for pair_kernel's wave path
    cnt = np.diff(want.rec_off.astype(np.int64))
    assert c["n_kind2"] >= 1 and len(kept) > c["n_kind2"] and c["n_unmapped"] >= 2 and c["n_proper"] >= 1
    assert any(cnt[i] * cnt[n + i] > K_PAIR_ALONE for i in range(n))
    return c


# ---- batches for the packed read forms: a small reference with planted repeats and near-copies, reads with edits on both
# strands, and reads carrying characters the packed form sends separately ----

UNIT, UNIT_COPIES = 300, 12
LONG_UNIT = 1500


def _clustered(rng, s, cluster, period):
    """A near-copy: `cluster` consecutive substitutions every `period` bases — a read over it is beyond e edits where a
    cluster of e + 2 falls inside it, and still shares whole seeds with the original between the clusters."""
    s = bytearray(s)
    for at in range(int(rng.integers(3, period)), len(s) - cluster, period):
        for i in range(at, at + cluster):
            s[i] = util.ACGT[(np.searchsorted(util.ACGT, s[i]) + 1 + rng.integers(0, 3)) % 4]
    return bytes(s)


def packed_reference(rng):
    """Four sequences of 20-60 kbp: a 300-base unit in 12 copies, three near-copies of it, a 1500-base unit twice with three
    near-copies (decoys for reads longer than the short unit), a 60-base repeat five times."""
    unit, long_unit, short = util.rand_seq(rng, UNIT), util.rand_seq(rng, LONG_UNIT), util.rand_seq(rng, 60)
    near = [(2, 14), (5, 30), (9, 45)]  # clusters of e + 2 for e = 0, 3, 7 (e = 1: two clusters of the first)
    pieces = [unit] * UNIT_COPIES + [_clustered(rng, unit, c, p) for c, p in near]
    pieces += [long_unit] * 2 + [_clustered(rng, long_unit, c, p) for c, p in near] + [short] * 5
    order = rng.permutation(len(pieces))
    seqs, places = [], []  # places: (sequence, offset, length) of the exact copies of the two units
    lens = [20_000, 35_000, 45_000, 60_000]
    per_seq = [[] for _ in lens]
    for j, pi in enumerate(order):
        per_seq[j % len(lens)].append(int(pi))
    for si, total in enumerate(lens):
        parts, used = [], 0
        gap = (total - sum(len(pieces[pi]) for pi in per_seq[si])) // (len(per_seq[si]) + 1)
        for pi in per_seq[si]:
            parts.append(util.rand_seq(rng, gap))
            used += gap
            if pi < UNIT_COPIES or len(pieces) - 5 - 3 - 2 <= pi < len(pieces) - 5 - 3:
                places.append((si, used, len(pieces[pi])))
            parts.append(pieces[pi])
            used += len(pieces[pi])
        parts.append(util.rand_seq(rng, total - used))
        seqs.append(b"".join(parts))
    return seqs, places


def _edit(rng, s, n_err, L):
    """n_err edits (substitutions, insertions, deletions) anywhere — the first and last three bases included."""
    s = bytearray(s)
    for _ in range(n_err):
        u = rng.random()
        pos = int(rng.integers(0, 3)) if u < 0.2 else L - 1 - int(rng.integers(0, 3)) if u < 0.4 else int(rng.integers(0, L))
        r = rng.random()
        if r < 0.6:
            s[pos] = util.ACGT[(np.searchsorted(util.ACGT, s[pos]) + 1 + rng.integers(0, 3)) % 4]
        elif r < 0.8:
            s.insert(pos, int(util.ACGT[rng.integers(0, 4)]))
        else:
            del s[pos]
    return bytes(s[:L])


def packed_reads(rng, seqs, places, n, L, e):
    """Half of the reads from inside the planted units (many candidates, decoys among them), half from anywhere; both
    strands; 0..e edits.  Reads 0 and n - 1 are exact and on the reverse strand: they load at the packed buffer's edges."""
    fit = [p for p in places if p[2] >= L + e]
    out = []
    for i in range(n):
        if fit and rng.random() < 0.5:
            si, at, ln = fit[int(rng.integers(0, len(fit)))]
            start = at + int(rng.integers(0, ln - (L + e) + 1))
        else:
            si = int(rng.integers(0, len(seqs)))
            start = int(rng.integers(0, len(seqs[si]) - (L + e) - 1))
        w = seqs[si][start:start + L + e]
        edge = i == 0 or i == n - 1
        r = w[:L] if edge else _edit(rng, w, int(rng.integers(0, e + 1)), L)
        out.append(util.revcomp(r) if edge or rng.random() < 0.5 else r)
    return out


def packed_exceptions(rng, reads, share):
    """A share of the reads carries one to three of N, n, a lower-case base and R, at the first, a middle and the last base.
    Returns the reads and, per read, 0 (untouched), 1 (lower-case bases only: same outcome as in upper case) or 2."""
    out, kind = [], np.zeros(len(reads), np.int8)
    for i, r in enumerate(reads):
        if rng.random() < share:
            r = bytearray(r)
            L = len(r)
            lower_only = rng.random() < 0.4
            places = [0, L // 2, L - 1]
            for at in [places[int(j)] for j in rng.permutation(3)[:int(rng.integers(1, 4))]]:
                r[at] = r[at] | 0x20 if lower_only else int(rng.choice([ord("N"), ord("n"), r[at] | 0x20, ord("R")]))
            kind[i] = 1 if lower_only else 2
            r = bytes(r)
        out.append(r)
    return out, kind


# ---- a reference for banks of sequences ----

def banked_reference(rng, n_seq, shared):
    """Sequences that share repeat units (a list then has entries in several banks) between stretches of their own."""
    units = [util.rand_seq(rng, 260) for _ in range(5)]
    seqs = []
    for s in range(n_seq):
        parts = [util.rand_seq(rng, int(rng.integers(200, 1500)))]
        for _ in range(int(rng.integers(18, 30))):
            if shared and rng.random() < 0.6:
                parts.append(util.mutate(rng, units[int(rng.integers(0, len(units)))], int(rng.integers(0, 3))))
            parts.append(util.rand_seq(rng, int(rng.integers(300, 2500))))
        if s % 3 == 1:
            parts.append(b"N" * 40)
            parts.append(util.rand_seq(rng, 900))
        seqs.append(b"".join(parts))
    return seqs


# ---- ragged batches with reads too short to seed (tests/test_gpu_dense_short_reads.py; the draw of tests/fuzz_gpu.py) ----

# (e, longest read): seed_select_kernel works on sub-blocks of 13, 8, 5, 5 and 2 reads at these (make_layout_select, fem_hip.hip)
SHORT_PARAMS = [(0, 64), (3, 100), (3, 150), (7, 150), (2, 300)]
SHORT_N = 17 * 16 * 2  # read r short iff r % 17 == 0: the short read visits every place of the 16-read block, twice
TOO_SHORT = 14         # lengths below this (0..13) have at most two 12-mers: the draw of tests/fuzz_gpu.py


def short_lengths(e):
    """No base, one, the last length whose unsigned L - (k - 1) wraps, the first that does not, one and two seeds, and one base
    under the shape gate of src/filter.c:5-7 at a = 1 (L - 11 - 2 >= 12 (e + 2): 37 + 12 e bases)."""
    return (0, 1, 10, 11, 12, 13, 36 + 12 * e)


@functools.lru_cache(maxsize=None)
def short_reads_reference():
    """A random sequence of 200 kbp with three units of 400 bases planted four times each (0..2 edits a copy), and a second
    sequence of ~21 kbp that holds each unit again: reads inside a unit have several hits, in both sequences (both banks).
    -> seqs, names, ref, idx."""
    rng = np.random.default_rng(1700)
    units = [util.rand_seq(rng, 400) for _ in range(3)]
    main, second = [], []
    for i in range(12):
        main += [util.rand_seq(rng, 16_266), util.mutate(rng, units[i % 3], int(rng.integers(0, 3)))]
    for u in units:
        second += [util.rand_seq(rng, 5_000), u]
    seqs = [b"".join(main), b"".join(second + [util.rand_seq(rng, 5_000)])]
    ref = fo.Reference(seqs)
    return seqs, ["chr0", "chr1"], ref, fo.OracleIndex(ref)


def every_17th_short(e, n=SHORT_N):
    ls = short_lengths(e)
    return {r: ls[(r // 17) % len(ls)] for r in range(0, n, 17)}


@functools.lru_cache(maxsize=None)
def short_reads_batch(seed, e, L, n=SHORT_N, short=None):
    """n reads: read r has short[r] bases where r is in `short` (a tuple of (read, length) pairs; None: every_17th_short), else
    L - 0..L/8 bases with 0..e edits, a third of them from inside the planted units; the first long read has exactly L bases (the
    kernels' layout follows the longest read).  Short reads are prefixes of reads that would map.  The oracle's result of the
    batch and of the batch without its short reads.  -> dict."""
    seqs, names, ref, idx = short_reads_reference()
    short = every_17th_short(e, n) if short is None else dict(short)
    rng = np.random.default_rng(seed)
    unit_at = [i * (16_266 + 400) + 16_266 for i in range(12)]  # (where the units start, but for the indels of earlier copies)
    reads, first_long = [], True
    for r in range(n):
        ln = short[r] if r in short else L if first_long else L - int(rng.integers(0, L // 8 + 1))
        first_long = first_long and r in short
        if r not in short and r % 3 == 0 and ln + e + 2 < 380:
            at = unit_at[int(rng.integers(0, 12))] + int(rng.integers(10, 380 - ln - e))
            read = util.mutate(rng, seqs[0][at:at + ln + e], int(rng.integers(0, e + 1)))[:ln]
            read = read + util.rand_seq(rng, ln - len(read))
            read = util.revcomp(read) if rng.random() < 0.5 else read
        else:
            read = util.make_reads(rng, seqs, 1, max(ln, 1), e if r not in short else 0)[0][:ln]
        assert len(read) == ln
        reads.append(read)
    long_reads = [x for r, x in enumerate(reads) if r not in short]
    want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    want_long = fo.map_reads(ref, idx, fo.ReadBatch(long_reads), e=e, threads=8) if long_reads else None
    return dict(reads=reads, short=sorted(short), e=e, L=L, want=want, want_long=want_long, rnames=["s%d" % r for r in range(n)],
                quals=quals(reads))


def per_read(res, n):
    """The oracle's result read by read: (candidates, edit distances and end offsets of both strands; FLAG, sequence, POS, NM,
    CIGAR and MD of its records), as bytes — what test_gpu_dense_short_reads.py compares between a batch and its long reads."""
    out = []
    for r in range(n):
        c0, c1 = int(res.cand_off[2 * r]), int(res.cand_off[2 * r + 2])
        mid = int(res.cand_off[2 * r + 1]) - c0
        ok = res.v_ed[c0:c1] != 0xFF
        j0, j1 = int(res.rec_off[r]), int(res.rec_off[r + 1])
        g0, g1, m0, m1 = int(res.cig_off[j0]), int(res.cig_off[j1]), int(res.md_off[j0]), int(res.md_off[j1])
        out.append((mid, res.cands[c0:c1].tobytes(), res.v_ed[c0:c1].tobytes(), res.v_end[c0:c1][ok].tobytes(),
                    res.r_flag[j0:j1].tobytes(), res.r_tid[j0:j1].tobytes(), res.r_pos[j0:j1].tobytes(), res.r_nm[j0:j1].tobytes(),
                    (res.cig_off[j0 + 1:j1 + 1] - res.cig_off[j0]).tobytes(), res.cig[g0:g1].tobytes(),
                    (res.md_off[j0 + 1:j1 + 1] - res.md_off[j0]).tobytes(), res.md[m0:m1].tobytes()))
    return out


# ---- solo regions of the join tests (tests/test_gpu_join_units.py, test_gpu_join_flags.py) ----

SOLO_SLOTS = 14                            # indexed 12-mers of a solo region: offsets 0, 3, .. 39 -> 51 bases
SOLO_LEN = 3 * (SOLO_SLOTS - 1) + 12


def lone_copies(rng, regions, which):
    """The 12-mers (class, slot) of `which`, each alone: three bases between one and the next, chosen so that none of the four
    indexed 12-mers across the joint is a 12-mer of a region again (the lists stay exactly as long as planned).  Twelve random
    bases in front and behind, joined the same way."""
    planted = {r[3 * j:3 * j + 12] for r in regions for j in range(SOLO_SLOTS)}
    mers = [util.rand_seq(rng, 12)] + [regions[c][3 * j:3 * j + 12] for c, j in which] + [util.rand_seq(rng, 12)]
    out = bytearray(mers[0])
    for nxt in mers[1:]:
        while True:
            joint = bytes(out[-12:]) + util.rand_seq(rng, 3) + nxt
            if not any(joint[o:o + 12] in planted for o in (3, 6, 9, 12)):
                break
        out += joint[12:]
    return bytes(out)


def over_home(rng, w, c, sq, pos, L, e):
    """A read of L bases that holds the whole solo region at (sq, pos), with 0..e edits in what lies before and behind the region
    (an edit inside it takes four of its seeds away, a gap the seed selection steps into: such reads say nothing here)."""
    s = w.seqs[sq]
    before = int(rng.integers(0, L - SOLO_LEN + 1))
    k = int(rng.integers(0, e + 1))
    k_left = int(rng.integers(0, k + 1)) if before >= 3 else 0
    left = util.mutate(rng, s[pos - before - e:pos], k_left)[-before:] if before else b""
    right = util.mutate(rng, s[pos + SOLO_LEN:pos + SOLO_LEN + L], k - k_left)
    return (left + s[pos:pos + SOLO_LEN] + right)[:L]


# ---- independent models of the banded edit distance and of the traceback (tests/test_oracle_models.py,
# test_traceback_model.py, test_rescue_host.py) ----

CODE = {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}


def code(c):
    return CODE.get(c, 4)  # src/utils.h:72


def banded_dp(e, pattern, text):
    """Edit distance of `text` against pattern[i+j], j in [0,2e] per column i; free start, free end, strict band."""
    INF = 10 ** 6
    L = len(text)
    prev = [0] * (2 * e + 1)
    score_path = 0
    for i in range(L):
        cur = [INF] * (2 * e + 1)
        for j in range(2 * e + 1):
            d = prev[j] + (0 if code(text[i]) == code(pattern[i + j]) else 1)
            h = prev[j + 1] + 1 if j + 1 <= 2 * e else INF
            v = cur[j - 1] + 1 if j >= 1 else INF
            cur[j] = min(d, h, v)
        prev = cur
        score_path = cur[0]
        if score_path > 3 * e:
            return e + 1, None
    best, end = prev[0], L - 1
    for j in range(1, 2 * e + 1):
        if prev[j] < best:
            best, end = prev[j], L - 1 + j
    return best, end


def banded_matrix(e, pattern, text):
    """D[t][j], t in 0..L-1, j in 0..2e, and the column before the first (all zero: free start)."""
    INF = 10 ** 6
    W = 2 * e + 1
    prev = [0] * W
    cols = []
    for t in range(len(text)):
        cur = [INF] * W
        for j in range(W):
            diag = prev[j] + (0 if code(text[t]) == code(pattern[t + j]) else 1)
            left = prev[j + 1] + 1 if j + 1 < W else INF  # (t-1, q) with q below the previous column's band
            up = cur[j - 1] + 1 if j >= 1 else INF
            cur[j] = min(diag, left, up)
        cols.append(cur)
        prev = cur
    return cols


def bits(e, cols, t, j):
    """(D0, HP) of cell (t, j) as the walk reads them."""
    W = 2 * e + 1
    prev = cols[t - 1] if t > 0 else [0] * W
    d0 = cols[t][j] == prev[j]
    left = prev[j + 1] if j + 1 < W else prev[j] + 1  # below the band the vertical step costs one (VP's high bits are set)
    hp = cols[t][j] - left == 1
    return d0, hp


class Asserted(Exception):
    pass


def model_align(e, pattern, text, ed, end):
    """-> (start, [(op, len)] left to right, md string); Asserted where the reference would trip an assert."""
    L = len(text)
    start = end - L + 1
    if start < 0:
        raise Asserted("start")
    if all(text[i] == pattern[start + i] for i in range(L)):  # raw characters (src/align.c:289-300)
        cigar = [("M", L)]
        return start, cigar, model_md(pattern, text, start, cigar)
    cols = banded_matrix(e, pattern, text)
    bit, t, p = end - L + 1, L - 1, end
    nerr = 0
    d0, hp = bits(e, cols, t, bit)
    if d0 and pattern[p] == text[t]:
        t, p, pre, n = t - 1, p - 1, "M", 1
    elif not d0:
        if pattern[p] == text[t]:
            raise Asserted("mismatch on equal characters")
        t, p, nerr, pre, n = t - 1, p - 1, nerr + 1, "S", 1
    elif d0 and hp:
        t, bit, nerr, pre, n, start = t - 1, bit + 1, nerr + 1, "S", 1, start + 1
    else:
        raise Asserted("deletion first")
    ops = []
    while t >= 0 and nerr != ed:
        if bit < 0 or bit > 2 * e:
            raise Asserted("off the band")
        d0, hp = bits(e, cols, t, bit)
        if d0 and pattern[p] == text[t]:
            t, p = t - 1, p - 1
            if pre != "M":
                ops.append((pre, n))
                pre, n = "M", 1
            else:
                n += 1
        elif not d0:
            if pattern[p] == text[t]:
                raise Asserted("mismatch on equal characters")
            t, p, nerr = t - 1, p - 1, nerr + 1
            if pre == "S":
                n += 1
            elif pre != "M":
                ops.append((pre, n))
                pre, n = "M", 1
            else:
                n += 1
        elif d0 and hp:
            t, bit, nerr, start = t - 1, bit + 1, nerr + 1, start + 1
            if pre == "S":
                n += 1
            elif pre != "I":
                ops.append((pre, n))
                pre, n = "I", 1
            else:
                n += 1
        else:
            bit, p, nerr, start = bit - 1, p - 1, nerr + 1, start - 1
            if pre != "D":
                ops.append((pre, n))
                pre, n = "D", 1
            else:
                n += 1
    if t >= 0:
        if pre != "M":
            ops.append((pre, n))
            ops.append(("M", t + 1))
        else:
            ops.append(("M", n + t + 1))
    else:
        ops.append((pre, n))
    if ops[0][0] == "S":
        if len(ops) < 2:
            raise Asserted("only the pseudo-run")
        ops[1] = (ops[1][0], ops[1][1] + ops[0][1])
        ops = ops[1:]
    if any(op == "S" for op, _ in ops):
        raise Asserted("S inside")
    cigar = ops[::-1]
    if start < 0:
        raise Asserted("start")
    return start, cigar, model_md(pattern, text, start, cigar)


def model_md(pattern, text, start, cigar):
    out, run, rp, tp = [], 0, start, 0
    for op, n in cigar:
        if op == "M":
            for _ in range(n):
                if pattern[rp] == text[tp]:
                    run += 1
                else:
                    if run:
                        out.append(str(run))
                        run = 0
                    out.append(chr(pattern[rp]))
                rp, tp = rp + 1, tp + 1
        elif op == "I":
            tp += n
        else:
            if run:
                out.append(str(run))
                run = 0
            out.append("^" + pattern[rp:rp + n].decode("latin-1"))
            rp += n
    if run:
        out.append(str(run))
    return "".join(out)


# ---- inputs and fingerprints of the comparison with the reference's klib (tests/test_ref_klib.py and
# tests/golden/make_klib_golden.py, which records what the reference returned for them) ----

def input_key(kind, data):
    return hashlib.sha1(kind + b"\0" + data).digest()[:8]


def file_key(path):
    data = open(path, "rb").read()
    return input_key(b"gz", gzip.decompress(data)) if data[:2] == b"\x1f\x8b" else input_key(b"raw", data)


def fingerprint(fields):
    """SHA-1 (first 16 bytes) of a sequence of byte strings, each with its length; None is told apart from b""."""
    h = hashlib.sha1()
    for f in fields:
        h.update(struct.pack("<q", -1 if f is None else len(f)))
        h.update(f or b"")
    return h.digest()[:16]


def view_fingerprints(records):
    """(names and sequences, qualities) of (name, sequence, quality) records: what same_records compares."""
    return (fingerprint([x for r in records for x in (r[0], r[1])]), fingerprint([r[2] for r in records]))


class StoredView:
    """The loader's view of kseq_read's records (loader_view) of a file, as klib_records.npz holds it: how many records,
    whether all have qualities, and the fingerprints of view_fingerprints."""

    def __init__(self, n, all_qual, names_seqs, quals):
        self.n, self.all_qual, self.names_seqs, self.quals = n, all_qual, names_seqs, quals

    def __len__(self):
        return self.n

    @classmethod
    def of(cls, view):
        ns, q = view_fingerprints([(r[0], r[2], r[3]) for r in view])
        all_qual = all(r[3] is not None for r in view)
        return cls(len(view), all_qual, ns, q if all_qual and view else bytes(16))  # (qualities compared only then)


def perm_fingerprint(perm):
    return fingerprint([np.ascontiguousarray(perm, dtype="<u4").tobytes()])


def loader_view(records, last_rc):
    """What load_batch_of_sequences_into_sequence_batch keeps (src/sequence_batch.c:47-66): zero-length records are
    skipped; a return value other than -1 at the end is "Didn't reach the end of sequence file" -> exit."""
    return [r for r in records if len(r[2]) > 0], last_rc != -1


HAND_MADE = {
    "four_line": b"@r1 first comment\nACGT\n+\nIIII\n@r2\tTAB comment\nGGCC\n+r2\n!!!!\n",
    "crlf": b"@r1 c\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nGG\r\n+\r\nJJ\r\n",
    "multi_line": b"@a\nACGT\nACG\n+\nIIII\nIII\n@b x\nTTTT\n+\nJJJJ\n",
    "fasta": b">s1 desc\nACGTACGT\nACGT\n>s2\nGG\n\n>s3\nTTTT",
    "mixed": b">f\nACGT\n@q\nGGGG\n+\nIIII\n>g\nCC\n",
    "at_plus_quals": b"@r1\nACGT\n+\n@+@+\n@r2\nACGT\n+\n+@+@\n@r3\nAC\n+\n@@\n",
    "blank_lines": b"\n\n@r1\nACGT\n+\nIIII\n\n\n@r2\nGG\n+\nII\n\n",
    "leading_junk": b"junk line\nmore junk\n@r1\nACGT\n+\nIIII\n",
    "no_final_newline": b"@r1\nACGT\n+\nIIII\n@r2\nGG\n+\nII",
    "zero_length": b"@e1\n\n+\n\n@r1\nACGT\n+\nIIII\n@e2\n\n+\n\n",
    "truncated_qual": b"@r1\nACGT\n+\nIIII\n@r2\nACGT\n+\nII\n",
    "missing_qual_at_eof": b"@r1\nACGT\n+\nIIII\n@r2\nACGT\n+\n",
    "header_only": b"@r1\n",
    "empty": b"",
    "only_newlines": b"\n\n\n",
    "lower_and_n": b"@r1\nacgtNNnn\n+\nIIIIIIII\n",
    "long_name": b"@" + b"n" * 300 + b" " + b"c" * 500 + b"\nACGT\n+\nIIII\n",
    "qual_longer": b"@r1\nACGT\n+\nIIIIII\n@r2\nGG\n+\nII\n",
    "plus_in_seq_line": b"@r1\nAC+GT\n+\nIIIII\n",
    "gt_in_fastq": b"@r1\nACGT\n+\nIIII\n>f1\nACGT\n@r2\nGG\n+\nII\n",
}


def random_file(rng):
    """FASTQ-like text with the irregularities kseq tolerates, then a few random byte edits."""
    out = []
    for i in range(int(rng.integers(1, 40))):
        ln = int(rng.integers(0, 70))
        seq = bytes(rng.choice(list(b"ACGTNacgt"), size=ln).astype(np.uint8))
        qual = bytes(rng.integers(33, 75, size=ln).astype(np.uint8))
        kind = rng.random()
        name = b"r%d" % i + (b" comment %d" % i if rng.random() < 0.5 else b"")
        eol = b"\r\n" if rng.random() < 0.1 else b"\n"
        if kind < 0.7:
            rec = b"@" + name + eol + seq + eol + b"+" + eol + qual + eol
        elif kind < 0.8 and ln > 4:  # multi-line
            h = ln // 2
            rec = b"@" + name + eol + seq[:h] + eol + seq[h:] + eol + b"+" + eol + qual[:h] + eol + qual[h:] + eol
        elif kind < 0.9:
            rec = b">" + name + eol + seq + eol
        else:
            rec = b"@" + name + eol + seq + eol + b"+" + name + eol + qual + eol + b"\n"
        out.append(rec)
    data = bytearray(b"".join(out))
    for _ in range(int(rng.integers(0, 3))):  # damage: delete, insert or change a byte
        if not data:
            break
        at = int(rng.integers(0, len(data)))
        op = rng.random()
        if op < 0.4:
            del data[at]
        elif op < 0.7:
            data.insert(at, int(rng.choice(list(b"@+>\nAI "))))
        else:
            data[at] = int(rng.choice(list(b"@+>\nAI ")))
    if rng.random() < 0.3 and data:
        data = data[:int(rng.integers(1, len(data) + 1))]  # cut off
    return bytes(data)


def sort_cases():
    rng = np.random.default_rng(77)
    cases = []
    for n in [0, 1, 2, 5, 63, 64, 65, 66, 100, 128, 129, 200, 257, 448, 1000, 5000]:
        for ties in (2, 8, 1 << 40):
            # MappingSortKey: edit distance << 60 | direction << 59 | position (src/align.c:53); few distinct values = many ties
            ed = rng.integers(0, 8, size=n).astype(np.uint64) << np.uint64(60)
            direction = rng.integers(0, 2, size=n).astype(np.uint64) << np.uint64(59)
            pos = rng.integers(0, ties, size=n).astype(np.uint64) * np.uint64(3 if ties < 100 else 1)
            cases.append(ed | direction | pos)
    return cases


# ---- read pairs that a cut makes mappable (tests/fuzz_lines.py) ----

CUT_PROFILES = ("good", "illumina", "walk", "plateau")  # the profiles of trim_model.profile_quals with printable bytes alone


def long_tail(e):
    """How many foreign bases on a read's 3' end keep the read as given from mapping at e edits.  A random base matches the
    reference with probability 1/4, so a tail of 8 bases stays within e >= 6 edits in most reads and within e = 2 in four of a
    thousand; 2e + 8 random bases have more than e mismatches in all but about 1e-4 of the reads at every e of 0 .. 7.  So
    cut_pairs makes no tail of 8 .. 2e + 7 bases: every made tail of 8 bases or more has this many."""
    return 2 * e + 8


def _subst(rng, s, k, lo=0, hi=None):
    """s with k substitutions at distinct places of [lo, hi)."""
    s = bytearray(s)
    hi = len(s) if hi is None else hi
    if hi > lo and k > 0:
        for p in rng.choice(hi - lo, min(k, hi - lo), replace=False):
            s[lo + int(p)] = b"ACGT"[(b"ACGT".index(bytes([s[lo + int(p)]])) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


def cut_pairs(rng, seqs, L, L2, e, flips=(0, 0), t5=0, t3=0, Q=0, A=None, A2=None, aO=5, aE=10, vO=None, vE=10, n=5):
    """Pairs that map only once they are cut, as the device is given them (mate 1 of L bases, mate 2 of L2): upper-case A C G T.
    Q > 0: n pairs with bad-quality tails (a reference segment, then 5 + 9k random bases under trim_model's "tail" profile).
    A: n pairs with adapter read-through (a segment, then a prefix of A, for mate 2 of A2, with a mismatch or two within aE).
    Those two kinds are pairs of an FR fragment of 150..500 bases, their flipped mates (flips: orient_model.FLIPS of the library)
    reverse-complemented first, so that the kept parts pair under the library's orientation.  One more pair with an adapter has a
    mate 1 that is all adapter behind its t5 bases: the match at p = 0, which keeps nothing.
    A or vO: pairs of a fragment of f < max(L, L2) bases, mate 1 the fragment, mate 2 its reverse complement, each read through
    into its adapter (where there is one) and random bases: the sequencer's geometry, whatever the library; f = max(L, L2) - 1 and
    f = vO among them, the others with 37 + 12e <= f; no f at which a mate reads 8 .. long_tail(e) - 1 bases through.
    vO: two pairs of such a fragment inside a tandem repeat, where several f match.
    The bodies carry 0..e substitutions; a tail is short (below 8 bases) or has long_tail(e) bases at the least, and where the
    read is long enough for it, it leaves 37 + 12e bases behind the fixed trims t5 and t3.
    -> dict(r1, r2, q1, q2: the mates and their quality strings; tails: per pair the foreign bases at (mate 1's, mate 2's) 3' end;
    seq: the sequence with the tandem repeat, to be added to the reference, or None)."""
    from tests import trim_model as trm
    main, lo, top, far = seqs[0], 37 + 12 * e, max(L, L2), long_tail(e)
    out = dict(r1=[], r2=[], q1=[], q2=[], tails=[], seq=None)

    def good(ln):
        return trm.profile_quals(rng, CUT_PROFILES[int(rng.integers(0, len(CUT_PROFILES)))], ln, int(rng.integers(0, 4))).decode("latin-1")

    def add(a, b, qa, qb, ta, tb):
        assert len(a) == len(qa) == L and len(b) == len(qb) == L2
        out["r1"].append(a), out["r2"].append(b), out["q1"].append(qa), out["q2"].append(qb), out["tails"].append((ta, tb))

    def fr_pair():
        frag = int(rng.integers(max(150, top), 501))
        st = int(rng.integers(0, len(main) - frag))
        f = main[st:st + frag] if rng.integers(0, 2) else util.revcomp(main[st:st + frag])
        a, b = f[:L], util.revcomp(f[frag - L2:])
        return (util.revcomp(a) if flips[0] else a), (util.revcomp(b) if flips[1] else b)

    def tail_length(ln):
        t = int(rng.integers(1, 8)) if rng.random() < 0.25 else far + int(rng.integers(0, 30))
        room = ln - lo - t5 - t3  # (the longest tail whose read still maps)
        return max(1, min(t, ln - 1, room if room >= far or t < 8 else t))

    for _ in range(n if Q > 0 else 0):
        mates, which = [], int(rng.integers(0, 3))  # the tail on mate 1, on mate 2, on both
        for m, body in enumerate(fr_pair()):
            ln = len(body)
            if which != 1 - m:
                k = 0 if rng.random() < 0.25 else -(-(far - 5) // 9) + int(rng.integers(0, 3))
                t = min(ln, 5 + 9 * k)
                body = _subst(rng, body[:ln - t], int(rng.integers(0, e + 1))) + util.rand_seq(rng, t)
                mates.append((body, trm.profile_quals(rng, "tail", ln, k).decode("latin-1"), t))
            else:
                mates.append((body, good(ln), 0))
        add(mates[0][0], mates[1][0], mates[0][1], mates[1][1], mates[0][2], mates[1][2])
    for _ in range(n if A else 0):
        mates, which = [], int(rng.integers(0, 3))
        for m, body in enumerate(fr_pair()):
            ln, ad = len(body), (A2 or A) if m else A
            t = tail_length(ln) if which != 1 - m else 0
            if t:
                o = min(t, len(ad))
                body = _subst(rng, body[:ln - t], int(rng.integers(0, e + 1))) + (ad + util.rand_seq(rng, ln))[:t]
                body = _subst(rng, body, min(int(rng.integers(0, 3)), o * aE // 100), ln - t, ln - t + o)
            mates.append((body, good(ln), t))
        add(mates[0][0], mates[1][0], mates[0][1], mates[1][1], mates[0][2], mates[1][2])
    if A:
        add((util.rand_seq(rng, t5) + A + util.rand_seq(rng, L))[:L], fr_pair()[1], good(L), good(L2), 0, 0)

    def through(fragment, k_body):
        f = len(fragment)
        fragment = _subst(rng, fragment, k_body)
        a = (fragment + (A or b"") + util.rand_seq(rng, L))[:L]
        b = (util.revcomp(fragment) + (A2 or A or b"") + util.rand_seq(rng, L2))[:L2]
        o = min(f, L) - max(0, f - L2)
        if vO is not None and o > 0:  # mate 1 against mate 2, within the mapping's e and the overlap's vE: in half of the pairs on it
            most = o * vE // 100
            k = most if most <= e - k_body and rng.integers(0, 2) else min(int(rng.integers(0, 3)), most, e - k_body)
            a = _subst(rng, a, k, max(0, f - L2), min(f, L))
        add(a, b, good(L), good(L2), max(0, L - f), max(0, L2 - f))

    def clear(f):
        """No mate of a fragment of f bases reads 8 .. long_tail(e) - 1 bases through it: such a read may or may not map as given."""
        return not any(8 <= ln - f < far for ln in (L, L2))

    if A or vO is not None:
        fs = [top - 1] + ([vO] if vO is not None and 1 <= vO < top else [])
        allowed = [f for f in range(lo, top) if clear(f)]
        fs += [int(allowed[int(rng.integers(0, len(allowed)))]) for _ in range(n)] if allowed else []
        fs += [top - t for t in (far, far + 1) if lo <= top - t]  # (the shortest read-through that keeps the read as given from mapping)
        for f in fs:
            if not clear(f):
                continue
            st = int(rng.integers(0, len(main) - f))
            fragment = main[st:st + f] if rng.integers(0, 2) else util.revcomp(main[st:st + f])
            through(fragment, int(rng.integers(0, e // 2 + 1)))
    if vO is not None:
        unit = util.rand_seq(rng, int(rng.choice([2, 3, 5, 7, 13])))
        repeat = (unit * 300)[:600]
        out["seq"] = util.rand_seq(rng, 300) + repeat + util.rand_seq(rng, 300)
        allowed = [f for f in range(min(lo, top - 1), top) if clear(f)]  # (top - 1 is among them: a tail of one base, or none)
        for _ in range(2):
            f = int(allowed[int(rng.integers(0, len(allowed)))])
            st = int(rng.integers(0, len(repeat) - f))
            through(repeat[st:st + f], 0)
    return out
