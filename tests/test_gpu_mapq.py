"""Mapping qualities on the device (fem_dev_set_mapq: mapq_kernel and pair_kernel<true> in front of the text kernels,
fem_tail.hip) against the plain-Python rule of tests/mapq_model.py on the oracle's records.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import mapq_model as mq
from tests import rescue_model as rm
from tests import util
from tests.cases import make_pairs, make_rescue_pairs, write_fastq
from tests.harness import bam_vs_sam, build_index, decode_bam_file, open_device, run_fem

pytestmark = pytest.mark.gpu



def _stage(dev, reads, rnames, quals, e, slot, quals_on_host=False):
    batch = fo.ReadBatch(reads)
    q = np.frombuffer("".join(quals).encode("latin-1"), np.uint8)
    dev.stage_reads(batch.bases, batch.off, slot=slot)
    dev.stage_text(q, rnames, slot=slot, quals_on_host=quals_on_host)
    dev.map_staged(e=e, slot=slot)
    return (q, batch.off) if quals_on_host else (None, None)


def _sam(dev, reads, rnames, quals, e, slot, quals_on_host=False, mapq=None):
    if mapq is not None:
        dev.set_mapq(mapq, slot=slot)
    q, off = _stage(dev, reads, rnames, quals, e, slot, quals_on_host)
    return dev.fetch_sam(slot=slot, quals=q, offsets=off)[0]


def _but_column5(text):
    return [l.split(b"\t")[:4] + l.split(b"\t")[5:] for l in text.splitlines()]


def _check(text_on, text_off, want):
    assert _but_column5(text_on) == _but_column5(text_off)
    assert mq.column5(text_on) == want
    assert mq.with_mapq(text_off, want) == text_on


@pytest.mark.parametrize("seed,e,L,n,repeats", [(1, 3, 100, 2000, False), (2, 3, 100, 1500, True), (3, 0, 100, 1500, True),
                                                 (4, 7, 150, 800, True), (5, 3, 300, 500, True), (6, 4, 1024, 200, False)])
def test_single_end_equals_the_model(seed, e, L, n, repeats):
    rng = np.random.default_rng(seed)
    if repeats:
        seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200)
        seqs.append(util.rand_seq(rng, 120_000))
    else:
        seqs = [util.rand_seq(rng, 200_000), util.rand_seq(rng, 50_000)]
    names = ["chr%d" % i for i in range(len(seqs))]
    reads = util.make_reads(rng, seqs, n, L, e, n_rate=0.003)
    rnames = ["read_%d_%s" % (i, "n" * (130 if i % 3 == 0 else i % 20)) for i in range(n)]  # names over 128 characters
    quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
    dev, ref, idx = open_device(seqs, names)
    try:
        res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
        want = mq.single_end(res, e)
        off = _sam(dev, reads, rnames, quals, e, 0)
        on = _sam(dev, reads, rnames, quals, e, 1, mapq=True)
        _check(on, off, want)
        assert len(set(want)) > 2 or e == 0
        # the qualities on the host: the fields the device leaves open move with the MAPQ's width
        assert _sam(dev, reads, rnames, quals, e, 1, quals_on_host=True) == on
        # BAM at both levels: the model's encoding of the MAPQ text
        _stage(dev, reads, rnames, quals, e, 1)
        bam_vs_sam(dev, 1, [x.encode() for x in names], n_sam=True)
        # off again: the bytes of a slot that never had it
        assert _sam(dev, reads, rnames, quals, e, 1, mapq=False) == off
    finally:
        dev.close()


def _pairs_case(seed, repeats):
    rng = np.random.default_rng(seed)
    if repeats:
        seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200)
        seqs.append(util.rand_seq(rng, 120_000))
    else:
        seqs = [util.rand_seq(rng, 200_000), util.rand_seq(rng, 60_000)]
    return rng, seqs, ["chr%d" % i for i in range(len(seqs))]


@pytest.mark.parametrize("seed,e,L,n,repeats", [(11, 3, 100, 1500, False), (12, 3, 100, 1000, True), (13, 7, 150, 600, True)])
def test_pairs_equal_the_model(seed, e, L, n, repeats):
    rng, seqs, names = _pairs_case(seed, repeats)
    r1, r2 = make_pairs(rng, seqs, n, L, e)
    reads = r1 + r2
    base = ["p%d_%s" % (i, "n" * (i % 140)) for i in range(n)]
    rnames = base + base
    quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
    dev, ref, idx = open_device(seqs, names)
    try:
        res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
        I, X = 0, 500
        dev.set_pairs(I, X, slot=1)
        off = _sam(dev, reads, rnames, quals, e, 1)
        on = _sam(dev, reads, rnames, quals, e, 1, mapq=True)
        want = mq.paired(res, n, e, I, X)
        _check(on, off, want)
        assert _sam(dev, reads, rnames, quals, e, 1, quals_on_host=True) == on
        _stage(dev, reads, rnames, quals, e, 1)
        bam_vs_sam(dev, 1, [x.encode() for x in names], n_sam=True)
        if repeats:  # pairs beyond kPairAlone combinations: pair_kernel's wave path
            counts = np.diff(res.rec_off.astype(np.int64))
            assert int((counts[:n] * counts[n:]).max()) > 32
        assert _sam(dev, reads, rnames, quals, e, 1, mapq=False) == off
    finally:
        dev.close()


@pytest.mark.parametrize("seed,repeats", [(21, False), (22, True)])
def test_rescued_pairs_equal_the_model(seed, repeats):
    rng, seqs, names = _pairs_case(seed, repeats)
    n, e, E, I, X = 1200, 2, 8, 0, 500
    r1, r2 = make_rescue_pairs(rng, seqs, n, 100, 100, e, E, X)
    reads = r1 + r2
    rnames = ["q%d" % i for i in range(n)] * 2
    quals = ["".join(chr(35 + (7 * i + j) % 50) for j in range(len(r))) for i, r in enumerate(reads)]
    dev, ref, idx = open_device(seqs, names)
    try:
        res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
        withr, kept, _ = rm.rescue(res, n, reads, seqs, E, I, X)
        assert kept
        dev.set_pairs(I, X, slot=2)
        dev.set_rescue(E, slot=2)
        off = _sam(dev, reads, rnames, quals, e, 2)
        on = _sam(dev, reads, rnames, quals, e, 2, mapq=True)
        _check(on, off, mq.paired(res, n, e, I, X, res=withr, rescued=set(kept)))
        _stage(dev, reads, rnames, quals, e, 2)
        bam_vs_sam(dev, 2, [x.encode() for x in names], n_sam=True)
    finally:
        dev.close()


def _diverged(rng, unit, windows):
    """unit with k distinct substitutions inside each window (lo, hi, k)."""
    u = bytearray(unit)
    for lo, hi, k in windows:
        for at in rng.choice(np.arange(lo, hi), size=k, replace=False):
            u[int(at)] = b"ACGT"[(b"ACGT".index(u[int(at)]) + int(rng.integers(1, 4))) % 4]
    return bytes(u)


def test_thousands_of_records_per_mate():
    # one 300-bp unit 1500 times, one copy exact and every other one with 2 or 3 substitutions inside each mate's window: mates
    # from the exact copy have a record in every copy (the wave paths of mapq_kernel and pair_kernel), their MAPQ rests on
    # exact counts: 512 copies with 2 substitutions under mate 1 (c2 = 512: Q(2, c2) = 13, 16 at 511), 256 under mate 2
    # (Q = 16), 128 with 2 under both (the concordant sum 4: Q(4, 128) = 59); pair: 53 and 56
    rng = np.random.default_rng(77)
    unit = util.rand_seq(rng, 300)
    parts = [util.rand_seq(rng, 50_000)]
    for c in range(1500):
        if c == 700:
            parts.append(unit)
        else:
            ka = 2 if c < 512 else 3
            kb = 2 if c < 128 or 512 <= c < 640 else 3
            parts.append(_diverged(rng, unit, [(3, 97, ka), (153, 247, kb)]))
        parts.append(util.rand_seq(rng, int(rng.integers(10, 50))))
    seqs = [b"".join(parts), util.rand_seq(rng, 200_000)]
    names = ["rep", "plain"]
    r1, r2 = make_pairs(rng, [seqs[1]], 200, 100, 3)
    a, b = unit[:100], util.revcomp(unit[150:250])
    r1[7], r2[7] = a, b
    r1[8], r2[8] = b, a
    r1[9] = a  # one mate in the repeat, the other elsewhere
    reads = r1 + r2
    rnames = ["q%d" % i for i in range(200)] * 2
    quals = ["I" * len(r) for r in reads]
    dev, ref, idx = open_device(seqs, names)
    try:
        res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=3, threads=8)
        assert np.diff(res.rec_off.astype(np.int64))[7] >= 1000
        dev.set_pairs(0, 500)
        on = _sam(dev, reads, rnames, quals, 3, 0, mapq=True)
        want = mq.paired(res, 200, 3, 0, 500)
        assert mq.column5(on) == want
        prim = {(l.split(b"\t")[0], int(l.split(b"\t")[1]) & 0xC0): int(l.split(b"\t")[4])
                for l in on.splitlines() if not int(l.split(b"\t")[1]) & 256}
        assert [prim[(b"q7", 0x40)], prim[(b"q7", 0x80)], prim[(b"q8", 0x40)], prim[(b"q8", 0x80)]] == [53, 56, 56, 53]
        dev.set_pairs(None)
        on = _sam(dev, reads, rnames, quals, 3, 0)
        want = mq.single_end(res, 3)
        assert mq.column5(on) == want
        col5 = mq.column5(on)  # (single-end lines in record order: read r's primary line is line rec_off[r])
        assert [col5[int(res.rec_off[r])] for r in (7, 207, 8, 208, 9)] == [13, 16, 16, 13, 13]
    finally:
        dev.close()


def _built_reference(rng):
    """Random sequence with its 2-kb stretch [20000, 22000) copied once at 60000 (more than X away)."""
    s = bytearray(util.rand_seq(rng, 100_000))
    s[60_000:62_000] = s[20_000:22_000]
    return [bytes(s)]


def test_by_construction():
    rng = np.random.default_rng(5)
    seqs = _built_reference(rng)
    s = seqs[0]
    dev, ref, idx = open_device(seqs, ["chrT"])
    try:
        inside = [s[x:x + 100] for x in (20_100, 20_700, 21_300)]
        unique = [s[x:x + 100] for x in (5_000, 40_000, 80_000)] + [util.revcomp(s[90_000:90_100])]
        reads = inside + unique
        rn = ["r%d" % i for i in range(len(reads))]
        text = _sam(dev, reads, rn, ["I" * 100] * len(reads), 3, 0, mapq=True)
        prim = [l.split(b"\t") for l in text.splitlines() if not int(l.split(b"\t")[1]) & 256]
        assert [int(f[4]) for f in prim] == [0, 0, 0, 60, 60, 60, 60]
        # a pair: mate 1 inside the copy, mate 2 in the unique flank behind it (insert 350)
        m1, m2 = s[21_800:21_900], util.revcomp(s[22_050:22_150])
        pr = [m1, m2]
        dev.set_pairs(0, 500, slot=1)
        text = _sam(dev, pr, ["pp", "pp"], ["I" * 100] * 2, 3, 1, mapq=True)
        prim = [l.split(b"\t") for l in text.splitlines() if not int(l.split(b"\t")[1]) & 256]
        assert [(int(f[1]) & 0xC2, int(f[4])) for f in prim] == [(0x42, 40), (0x82, 60)]
        text = _sam(dev, pr, ["pp", "pp"], ["I" * 100] * 2, 3, 0)
        assert [int(l.split(b"\t")[4]) for l in text.splitlines() if not int(l.split(b"\t")[1]) & 256] == [0, 60]
    finally:
        dev.close()


def test_kernel_time_ids():
    rng = np.random.default_rng(8)
    seqs = [util.rand_seq(rng, 100_000)]
    reads = util.make_reads(rng, seqs, 300, 100, 3)
    rn = ["r%d" % i for i in range(300)]
    quals = ["I" * 100] * 300
    dev, ref, idx = open_device(seqs, ["c"])
    try:
        dev.set_timing(True)
        for on, pairs in ((False, False), (True, False), (True, True)):
            dev.set_mapq(on)
            dev.set_pairs(0, 500) if pairs else dev.set_pairs(None)
            dev.reset_timing()
            for k in range(2):
                _stage(dev, reads, rn, quals, 3, 0)
                dev.fetch_sam()
                _stage(dev, reads, rn, quals, 3, 0)
                dev.fetch_bam(level=0)
            assert dev.kernel_time(13)[1] == (4 if on else 0)
            assert all(dev.kernel_time(i)[1] == 4 for i in (3, 4, 5))
            assert dev.kernel_time(9)[1] == (4 if pairs else 0)
    finally:
        dev.close()


# ---- FEM map --mapq ----

def _acgt_reference(rng):
    """Random sequences with a few units copied many times (no N: every rule input is in the text)."""
    units = [util.rand_seq(rng, 400) for _ in range(3)]
    parts = [util.rand_seq(rng, 5000)]
    for k in range(30):
        parts.append(util.mutate(rng, units[k % 3], int(rng.integers(0, 3))))
        parts.append(util.rand_seq(rng, int(rng.integers(200, 2000))))
    return [b"".join(parts), util.rand_seq(rng, 120_000)]


def _map(*args, env=None):
    return run_fem("map", *args, env=env)


def _body(data):
    return b"".join(l + b"\n" for l in data.splitlines() if not l.startswith(b"@"))


def test_cli(tmp_path):
    rng = np.random.default_rng(61)
    seqs = _acgt_reference(rng)
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = str(tmp_path / "ref.idx")
    build_index(fa, idx_path)
    n = 2000
    se = util.make_reads(rng, seqs, n, 100, 3)
    r1, r2 = make_pairs(rng, seqs, n, 100, 3)
    x1, x2 = make_rescue_pairs(rng, seqs, n, 100, 100, 3, 4, 500, frac=0.2)
    q = ["".join(chr(33 + (7 * i + j) % 40) for j in range(100)) for i in range(n)]
    files = {}
    for key, reads, suffix in (("se", se, ""), ("r1", r1, "/1"), ("r2", r2, "/2"), ("x1", x1, "/1"), ("x2", x2, "/2")):
        files[key] = tmp_path / (key + ".fq")
        write_fastq(files[key], reads, ["r%d%s" % (i, suffix) for i in range(n)], q, False)
    common = ["-e", "3", "-t", "4", "--ref", str(fa), "--index", idx_path, "--batch", "700"]
    share = {"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"}
    cases = [("se", ["--read1", str(files["se"])], False, True, None),
             ("pairs", ["--read1", str(files["r1"]), "--read2", str(files["r2"])], True, True, None),
             ("rescue", ["--read1", str(files["x1"]), "--read2", str(files["x2"]), "--rescue", "4"], True, False, None),
             ("gpus", ["--read1", str(files["r1"]), "--read2", str(files["r2"]), "--gpus", "2"], True, True, share),
             ("hostq", ["--read1", str(files["se"])], False, True, {"FEM_HOST_QUALS": "1"})]
    for name, args, paired, model, env in cases:
        off, on = str(tmp_path / (name + ".off.sam")), str(tmp_path / (name + ".on.sam"))
        r = _map(*(common + args + ["-o", off]), env=env)
        assert r.returncode == 0, r.stderr.decode()
        r = _map(*(common + args + ["-o", on, "--mapq"]), env=env)
        assert r.returncode == 0, r.stderr.decode()
        a, b = open(off, "rb").read(), open(on, "rb").read()
        if name == "gpus":  # batches in completion order (a pair's lines stay together): compared modulo line order
            assert sorted(_body(b).splitlines()) == sorted(mq.with_mapq(_body(a), mq.from_sam(a, 3, True)).splitlines())
            continue
        assert _but_column5(b) == _but_column5(a), name
        if model:
            assert mq.column5(b) == mq.from_sam(a, 3, paired), name
        assert len(set(mq.column5(b))) > 2, name
        assert set(mq.column5(a)) == {255}
        if name == "rescue":
            assert any("rescued" in l for l in r.stderr.decode().splitlines())
    # BAM: decodes to the --mapq SAM
    out = str(tmp_path / "on.bam")
    r = _map(*(common + ["--read1", str(files["r1"]), "--read2", str(files["r2"]), "-o", out, "--mapq", "--bam"]))
    assert r.returncode == 0, r.stderr.decode()
    assert decode_bam_file(out) == open(str(tmp_path / "pairs.on.sam"), "rb").read()
