"""Paired-end mapping on the device (fem_dev_set_pairs: pair_kernel + the SAM kernels in pair order, fem_tail.hip) against the
plain-Python model of tests/pair_model.py on the oracle's single-end records.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import pair_model as pm
from tests import util
from tests.cases import make_pairs, write_fastq
from tests.harness import build_index, counters, fetch_sam, open_device, open_reference, run_fem, same_pairs

pytestmark = pytest.mark.gpu


def _setup(seed, repeats, long_fields=False):
    return open_reference(seed, repeats, 50_000, 70 if long_fields else 7)


def _fields(text):
    """SAM lines split into fields, SEQ (which goes through the 4-bit BAM round trip) aside."""
    return [l.split("\t")[:9] + l.split("\t")[10:] for l in text.splitlines()]


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
        text, n_records, n_asserted, stats = fetch_sam(dev, reads, rnames, quals, e, slot=1)
        assert np.array_equal(stats, want.stats) and n_records == int(want.rec_off[-1])
        exp = pm.sam_lines(want, n, names, reads, rnames, quals, I, X)
        assert _fields(text.decode("latin-1")) == _fields(exp)
        if seed != 1:
            assert text.decode("latin-1") == exp
        _, n_proper = pm.expected(want, n, I, X)
        assert dev.pair_count(slot=1) == n_proper
        assert n_proper > n // 5 or L < 40
        # the qualities kept on the host: the same bytes
        text_h, _, _, _ = fetch_sam(dev, reads, rnames, quals, e, slot=1, quals_on_host=True)
        assert text_h == text
        # fetch_pairs: the model's arrays
        same_pairs(dev.fetch_pairs(slot=1), pm.pair_arrays(want, n, I, X))
        # invariant: a mate's lines without the mate bits and columns are its single-end lines
        rec = dev.fetch_records(slot=1)
        strip = lambda l: tuple(l[:1] + [str(int(l[1]) & 16)] + l[2:6] + l[11:])
        single = sorted(strip(l.split("\t")) for l in _single_end_text(rec, names, rnames).splitlines())
        paired = sorted(strip(l.split("\t")) for l in text.decode("latin-1").splitlines())
        assert paired == single
        # single-end again: byte-identical to a slot that never was in pair mode
        dev.set_pairs(None, slot=1)
        text_se, _, _, _ = fetch_sam(dev, reads, rnames, quals, e, slot=1)
        text_0, _, _, _ = fetch_sam(dev, reads, rnames, quals, e, slot=0)
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
    dev, ref, idx = open_device(seqs, names)
    try:
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
        text, _, _, _ = fetch_sam(dev, reads, rnames, quals, 3)
        assert text.decode("latin-1") == pm.sam_lines(want, 300, names, reads, rnames, quals, 0, 500)
        same_pairs(dev.fetch_pairs(), pm.pair_arrays(want, 300, 0, 500))
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
        same_pairs(dev.fetch_pairs(), pm.pair_arrays(want, n, 100, 550))
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
            fetch_sam(dev, reads, rnames, quals, 3)
        with pytest.raises(FemError):
            dev.fetch_pairs()
    finally:
        dev.close()


# ---- FEM map --read1 --read2 ----

def _cli_case(tmp_path, seed, n, gz, suffix, batch=None):
    rng = np.random.default_rng(seed)
    seqs = [util.rand_seq(rng, 150_000), util.rand_seq(rng, 60_000)]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = tmp_path / "ref.idx"
    build_index(fa, idx_path)
    r1, r2 = make_pairs(rng, seqs, n, 100, 3)
    base = ["pair%d" % i for i in range(n)]
    q1 = ["".join(chr(33 + (7 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r1)]
    q2 = ["".join(chr(34 + (5 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r2)]
    ext = ".fq.gz" if gz else ".fq"
    p1, p2 = tmp_path / ("r1" + ext), tmp_path / ("r2" + ext)
    write_fastq(p1, r1, [b + ("/1" if suffix else "") for b in base], q1, gz)
    write_fastq(p2, r2, [b + ("/2" if suffix else "") for b in base], q2, gz)
    ref = fo.Reference(seqs)
    want = fo.map_reads(ref, fo.OracleIndex(ref), fo.ReadBatch(r1 + r2), e=3, threads=4)
    header = "".join("@SQ\tSN:s%d\tLN:%d\n" % (i, len(s)) for i, s in enumerate(seqs))
    exp = header + pm.sam_lines(want, n, ["s0", "s1"], r1 + r2, base + base, q1 + q2, 0, 500)
    return fa, idx_path, p1, p2, want, exp


def _map(fa, idx_path, p1, p2, out, *extra, env=None):
    return run_fem("map", "-e", "3", "-t", "4", "--ref", fa, "--index", idx_path, "--read1", p1, "--read2", p2, "-o", out, *extra,
                   env=env, text=True)


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
    assert counters(r.stderr) == ["The number of read: %d" % st[0], "The number of mapped read: %d" % st[1],
                                   "The number of candidate before additional q-gram filter: %d" % st[2],
                                   "The number of candidate: %d" % st[3], "The number of mapping: %d" % st[4],
                                   "The number of proper pairs: %d" % n_proper]
    # the qualities kept on the host (-t 24): the same bytes
    out24 = tmp_path / "out24.sam"
    r = run_fem("map", "-e", "3", "-t", "24", "--ref", fa, "--index", idx_path, "--read1", p1, "--read2", p2, "-o", out24,
                "--batch", "1000", text=True)
    assert r.returncode == 0, r.stderr
    assert out24.read_bytes() == out.read_bytes()
    # two workers sharing GPU 0: the same lines, batches in completion order
    out2 = tmp_path / "out2.sam"
    r = _map(fa, idx_path, p1, p2, out2, "--batch", "1000", "--gpus", "2", env={"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"})
    assert r.returncode == 0, r.stderr
    assert sorted(out2.read_text(encoding="latin-1").splitlines()) == sorted(exp.splitlines())
    assert counters(r.stderr)[-1] == "The number of proper pairs: %d" % n_proper


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
