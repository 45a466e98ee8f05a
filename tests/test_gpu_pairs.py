"""Paired-end mapping on the device (fem_dev_set_pairs: pair_kernel + the SAM kernels in pair order, fem_tail.hip) against the
plain-Python model of tests/pair_model.py on the oracle's single-end records.  Needs a GPU: -m gpu."""
import os
import subprocess

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import pair_model as pm
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEM = os.path.join(ROOT, "fem_amd", "csrc", "FEM")


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


def _setup(seed, repeats, long_fields=False):
    from fem_amd import Device
    rng = np.random.default_rng(seed)
    if repeats:
        seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200)
        seqs.append(util.rand_seq(rng, 120_000))
    else:
        seqs = [util.rand_seq(rng, 200_000), util.rand_seq(rng, 50_000)]
    names = ["chr%d_%s" % (i, "x" * (i * (70 if long_fields else 7))) for i in range(len(seqs))]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    dev = Device(0)
    dev.upload_reference(seqs)
    dev.upload_reference_names(names)
    dev.upload_index(12, 3, idx.lookup, idx.occ[:idx.n_occ])
    return rng, dev, ref, idx, seqs, names


def _run(dev, reads, rnames, quals, e, slot=0, quals_on_host=False):
    batch = fo.ReadBatch(reads)
    q = np.frombuffer("".join(quals).encode("latin-1"), np.uint8)
    dev.stage_reads(batch.bases, batch.off, slot=slot)
    dev.stage_text(q, rnames, slot=slot, quals_on_host=quals_on_host)
    dev.map_staged(e=e, slot=slot)
    if quals_on_host:
        return dev.fetch_sam(slot=slot, quals=q, offsets=batch.off)
    return dev.fetch_sam(slot=slot)


def _fields(text):
    """SAM lines split into fields, SEQ (which goes through the 4-bit BAM round trip) aside."""
    return [l.split("\t")[:9] + l.split("\t")[10:] for l in text.splitlines()]


def _same_pairs(got, want):
    for k, v in want.items():
        if k == "n_proper":
            assert got.n_proper == v
        else:
            assert np.array_equal(getattr(got, k), v), k


@pytest.mark.parametrize("seed,e,L,L2,n,repeats,long_fields", [
    (1, 3, 100, 100, 1500, False, False), (2, 7, 150, 150, 800, True, False), (3, 2, 64, 64, 2000, True, False),
    (4, 0, 36, 36, 500, False, False), (5, 3, 260, 260, 500, False, True), (6, 3, 100, 75, 1000, True, False)])
def test_paired_text_equals_the_model(seed, e, L, L2, n, repeats, long_fields):
    rng, dev, ref, idx, seqs, names = _setup(seed, repeats, long_fields)
    try:
        r1, r2 = make_pairs(rng, seqs, n, L, e, L2)
        if seed == 1:  # odd characters in a few mates
            r1[3] = r1[3].lower()
            r2[5] = r2[5][:L // 2] + b"RYKM=.-*" + r2[5][L // 2 + 8:]
        reads = r1 + r2
        base = ["p%d_%s" % (i, "n" * (i % (150 if long_fields else 40))) for i in range(n)]
        rnames = base + base
        quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
        want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e)
        I, X = 0, 500 if seed != 2 else 300
        dev.set_pairs(I, X, slot=1)
        text, n_records, n_asserted, stats = _run(dev, reads, rnames, quals, e, slot=1)
        assert np.array_equal(stats, want.stats) and n_records == int(want.rec_off[-1])
        exp = pm.sam_lines(want, n, names, reads, rnames, quals, I, X)
        assert _fields(text.decode("latin-1")) == _fields(exp)
        if seed != 1:
            assert text.decode("latin-1") == exp
        _, n_proper = pm.expected(want, n, I, X)
        assert dev.pair_count(slot=1) == n_proper
        assert n_proper > n // 5 or L < 40
        # the qualities kept on the host: the same bytes
        text_h, _, _, _ = _run(dev, reads, rnames, quals, e, slot=1, quals_on_host=True)
        assert text_h == text
        # fetch_pairs: the model's arrays
        _same_pairs(dev.fetch_pairs(slot=1), pm.pair_arrays(want, n, I, X))
        # invariant: a mate's lines without the mate bits and columns are its single-end lines
        rec = dev.fetch_records(slot=1)
        strip = lambda l: tuple(l[:1] + [str(int(l[1]) & 16)] + l[2:6] + l[11:])
        single = sorted(strip(l.split("\t")) for l in _single_end_text(rec, names, rnames).splitlines())
        paired = sorted(strip(l.split("\t")) for l in text.decode("latin-1").splitlines())
        assert paired == single
        # single-end again: byte-identical to a slot that never was in pair mode
        dev.set_pairs(None, slot=1)
        text_se, _, _, _ = _run(dev, reads, rnames, quals, e, slot=1)
        text_0, _, _, _ = _run(dev, reads, rnames, quals, e, slot=0)
        assert text_se == text_0
    finally:
        dev.close()


def _single_end_text(rec, seq_names, rnames):
    out = []
    for r in range(rec.n_reads):
        for j in range(int(rec.rec_begin[r]), int(rec.rec_begin[r + 1])):
            ops = rec.cigar[int(rec.cigar_off[j]):int(rec.cigar_off[j + 1])]
            cig = "".join("%d%s" % (int(o) >> 4, "MID"[int(o) & 0xF]) for o in ops) or "*"
            md = rec.md[int(rec.md_off[j]):int(rec.md_off[j + 1])].tobytes().decode()
            out.append("\t".join([rnames[r], str(int(rec.flag[j]) & 0x7FFF), seq_names[int(rec.tid[j])], str(int(rec.pos0[j]) + 1),
                                  "255", cig, "*", "0", "0", "-", "-", "NM:i:%d" % int(rec.nm[j]), "MD:Z:" + md]))
    return "".join(l + "\n" for l in out)


def test_thousands_of_records_per_mate():
    from fem_amd import Device
    # one 300-bp unit ~2500 times (as test_gpu_tail.py::test_thousands_of_mappings_per_read): both mates inside it have
    # records in every copy, millions of combinations per pair, the wave-wide path of pair_kernel
    rng = np.random.default_rng(77)
    unit = util.rand_seq(rng, 300)
    parts = [util.rand_seq(rng, 50_000)]
    for _ in range(2500):
        parts.append(util.mutate(rng, unit, int(rng.integers(0, 2))))
        parts.append(util.rand_seq(rng, int(rng.integers(10, 50))))
    seqs = [b"".join(parts), util.rand_seq(rng, 200_000)]
    names = ["rep", "plain"]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    dev = Device(0)
    try:
        dev.upload_reference(seqs)
        dev.upload_reference_names(names)
        dev.upload_index(12, 3, idx.lookup, idx.occ[:idx.n_occ])
        r1, r2 = make_pairs(rng, [seqs[1]], 300, 100, 3)
        a, b = unit[:100], util.revcomp(unit[150:250])
        r1[7], r2[7] = a, b
        r1[8], r2[8] = b, a
        r1[9], r2[9] = a, r2[9]  # one mate in the repeat, the other elsewhere
        reads = r1 + r2
        rnames = ["q%d" % i for i in range(300)] * 2
        quals = ["I" * len(r) for r in reads]
        want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=3, threads=8)
        counts = np.diff(want.rec_off.astype(np.int64))
        assert counts[7] >= 1000 and counts[300 + 7] >= 1000
        dev.set_pairs(0, 500)
        text, _, _, _ = _run(dev, reads, rnames, quals, 3)
        assert text.decode("latin-1") == pm.sam_lines(want, 300, names, reads, rnames, quals, 0, 500)
        _same_pairs(dev.fetch_pairs(), pm.pair_arrays(want, 300, 0, 500))
    finally:
        dev.close()


def test_a_large_batch_equals_the_model():
    rng, dev, ref, idx, seqs, names = _setup(12, False)
    try:
        n = 100_000
        r1, r2 = make_pairs(rng, seqs, n, 50, 2)
        reads = r1 + r2
        want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=2, threads=8)
        batch = fo.ReadBatch(reads)
        dev.set_pairs(100, 550)
        dev.stage_reads(batch.bases, batch.off)
        dev.map_staged(e=2)
        _same_pairs(dev.fetch_pairs(), pm.pair_arrays(want, n, 100, 550))
    finally:
        dev.close()


def test_refusals():
    from fem_amd import FemError
    rng, dev, ref, idx, seqs, names = _setup(13, False)
    try:
        r1, r2 = make_pairs(rng, seqs, 20, 100, 3)
        reads = r1 + r2[:-1]  # an odd number of reads
        quals = ["I" * len(r) for r in reads]
        rnames = ["o%d" % i for i in range(len(reads))]
        with pytest.raises(FemError):
            dev.fetch_pairs()  # not in pair mode
        for bad in ((-1, 500), (600, 500), (0, (1 << 30) + 1)):
            with pytest.raises(FemError):
                dev.set_pairs(*bad)
        dev.set_pairs(0, 1 << 30)
        with pytest.raises(FemError):
            _run(dev, reads, rnames, quals, 3)
        with pytest.raises(FemError):
            dev.fetch_pairs()
    finally:
        dev.close()


# ---- FEM map --read1 --read2 ----

def _write_fastq(path, reads, names, quals, gz):
    import gzip
    data = "".join("@%s comment\n%s\n+\n%s\n" % (n, r.decode("latin-1"), q) for n, r, q in zip(names, reads, quals)).encode("latin-1")
    if gz:
        with gzip.open(str(path), "wb") as f:
            f.write(data)
    else:
        path.write_bytes(data)


def _cli_case(tmp_path, seed, n, gz, suffix, batch=None):
    rng = np.random.default_rng(seed)
    seqs = [util.rand_seq(rng, 150_000), util.rand_seq(rng, 60_000)]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = tmp_path / "ref.idx"
    subprocess.run([FEM, "index", "12", "3", str(fa), str(idx_path)], check=True, capture_output=True, timeout=600)
    r1, r2 = make_pairs(rng, seqs, n, 100, 3)
    base = ["pair%d" % i for i in range(n)]
    q1 = ["".join(chr(33 + (7 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r1)]
    q2 = ["".join(chr(34 + (5 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r2)]
    ext = ".fq.gz" if gz else ".fq"
    p1, p2 = tmp_path / ("r1" + ext), tmp_path / ("r2" + ext)
    _write_fastq(p1, r1, [b + ("/1" if suffix else "") for b in base], q1, gz)
    _write_fastq(p2, r2, [b + ("/2" if suffix else "") for b in base], q2, gz)
    ref = fo.Reference(seqs)
    want = fo.map_reads(ref, fo.OracleIndex(ref), fo.ReadBatch(r1 + r2), e=3, threads=4)
    header = "".join("@SQ\tSN:s%d\tLN:%d\n" % (i, len(s)) for i, s in enumerate(seqs))
    exp = header + pm.sam_lines(want, n, ["s0", "s1"], r1 + r2, base + base, q1 + q2, 0, 500)
    return fa, idx_path, p1, p2, want, exp


def _map(fa, idx_path, p1, p2, out, *extra, env=None):
    e = dict(os.environ, **(env or {}))
    return subprocess.run([FEM, "map", "-e", "3", "-t", "4", "--ref", str(fa), "--index", str(idx_path), "--read1", str(p1),
                           "--read2", str(p2), "-o", str(out)] + list(extra), capture_output=True, text=True, env=e, timeout=900)


def _counters(stderr):
    return [l for l in stderr.splitlines() if l.startswith("The number of")]


@pytest.mark.parametrize("gz,suffix", [(False, True), (True, False)])
def test_cli_paired_output_equals_the_model(tmp_path, gz, suffix):
    n = 3000
    fa, idx_path, p1, p2, want, exp = _cli_case(tmp_path, 21 + gz, n, gz, suffix)
    out = tmp_path / "out.sam"
    r = _map(fa, idx_path, p1, p2, out, "--batch", "1000")
    assert r.returncode == 0, r.stderr
    assert out.read_text(encoding="latin-1") == exp
    st = want.stats
    _, n_proper = pm.expected(want, n, 0, 500)
    assert _counters(r.stderr) == ["The number of read: %d" % st[0], "The number of mapped read: %d" % st[1],
                                   "The number of candidate before additional q-gram filter: %d" % st[2],
                                   "The number of candidate: %d" % st[3], "The number of mapping: %d" % st[4],
                                   "The number of proper pairs: %d" % n_proper]
    # the qualities kept on the host (-t 24): the same bytes
    out24 = tmp_path / "out24.sam"
    r = subprocess.run([FEM, "map", "-e", "3", "-t", "24", "--ref", str(fa), "--index", str(idx_path), "--read1", str(p1),
                        "--read2", str(p2), "-o", str(out24), "--batch", "1000"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    assert out24.read_bytes() == out.read_bytes()
    # two workers sharing GPU 0: the same lines, batches in completion order
    out2 = tmp_path / "out2.sam"
    r = _map(fa, idx_path, p1, p2, out2, "--batch", "1000", "--gpus", "2", env={"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"})
    assert r.returncode == 0, r.stderr
    assert sorted(out2.read_text(encoding="latin-1").splitlines()) == sorted(exp.splitlines())
    assert _counters(r.stderr)[-1] == "The number of proper pairs: %d" % n_proper


def test_cli_refuses_bad_pairs(tmp_path):
    fa, idx_path, p1, p2, want, exp = _cli_case(tmp_path, 31, 200, False, True)
    out = tmp_path / "out.sam"
    lines = p2.read_text().splitlines(True)
    bad = tmp_path / "bad_names.fq"
    bad.write_text("".join(lines[:8]) + "@other\n" + "".join(lines[9:]))
    r = _map(fa, idx_path, p1, bad, out)
    assert r.returncode == 1 and "Read names differ in the two read files: pair2 other" in r.stderr
    short = tmp_path / "short.fq"
    short.write_text("".join(lines[:-4]))
    r = _map(fa, idx_path, p1, short, out)
    assert r.returncode == 1 and "The two read files hold different numbers of reads." in r.stderr
    r = _map(fa, idx_path, p2, p1, out, env={"FEM_HOST_FORMAT": "1"})
    assert r.returncode == 1 and "FEM_HOST_FORMAT" in r.stderr
