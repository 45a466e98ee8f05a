"""Lines for unmapped reads on the device (fem_dev_set_unmapped: the line index kernels and the kUnm instances of the text and
BAM record kernels, fem_tail.hip) against the plain-Python rule of tests/unmapped_model.py on the oracle's records, and against
the device's own default output.  Needs a GPU: -m gpu.  (The case generators below are also run without one, by
tests/test_unmapped_model.py: they must give enough unmapped reads of every kind.)"""
import os
import subprocess

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import rescue_model as rm
from tests import unmapped_model as um
from tests import util
from tests.test_gpu_bam import _bam_vs_sam, _decode_bam_file
from tests.test_gpu_pairs import _write_fastq, make_pairs
from tests.test_gpu_rescue import make_rescue_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEM = os.path.join(ROOT, "fem_amd", "csrc", "FEM")
I, X = 0, 500


# ---- the cases: unmapped reads by construction (reads of random letters, reads with more than e edits) ----

def _reference(rng, repeats):
    if repeats:
        seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200)
        seqs.append(util.rand_seq(rng, 120_000))
    else:
        seqs = [util.rand_seq(rng, 200_000), util.rand_seq(rng, 60_000)]
    return seqs, ["chr%d" % i for i in range(len(seqs))]


def _quals(reads):
    return ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]


# seed, e, L, n, repeat-rich reference, odd reads (lengths, letters, N runs, a read of length 0)
SINGLE_CASES = [(101, 3, 100, 1500, False, True), (102, 3, 100, 1200, True, False), (103, 7, 150, 600, True, True),
                (104, 0, 64, 800, False, False)]


def single_case(seed, e, L, n, repeats, odd):
    rng = np.random.default_rng(seed)
    seqs, names = _reference(rng, repeats)
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
    return dict(seqs=seqs, names=names, reads=reads, rnames=rnames, quals=_quals(reads), e=e, ref=ref, idx=idx, res=res,
                repeats=repeats, odd=odd)


def check_single_case(c):
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
PAIR_CASES = [(111, 3, 100, 900, False, None), (112, 3, 100, 700, True, None), (113, 2, 100, 700, False, 8),
              (114, 2, 100, 600, True, 8)]


def pair_case(seed, e, L, n, repeats, E):
    rng = np.random.default_rng(seed)
    seqs, names = _reference(rng, repeats)
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
    return dict(seqs=seqs, names=names, reads=reads, rnames=base + base, quals=_quals(reads), e=e, E=E, n=n, ref=ref, idx=idx,
                res=res, withr=withr, kept=kept)


def check_pair_case(c):
    n, after = c["n"], c["withr"] if c["withr"] is not None else c["res"]
    assert min(um.pair_classes(c["res"], n)) >= 20, um.pair_classes(c["res"], n)
    n_unm = len(um.unmapped_reads(after, 2 * n))
    assert 0.05 * 2 * n <= n_unm <= 0.95 * 2 * n
    if c["E"] is not None:
        assert len(c["kept"]) >= 20 and min(um.pair_classes(after, n)) >= 20
        lost = [r for r in um.unmapped_reads(after, 2 * n) if int(after.rec_off[(r + n) % (2 * n) + 1]) > int(after.rec_off[(r + n) % (2 * n)])]
        assert len(lost) >= 20  # mates that stay unmapped beside a mapped one


# ---- the device ----

def _device(c):
    from fem_amd import Device
    dev = Device(0)
    dev.upload_reference(c["seqs"])
    dev.upload_reference_names(c["names"])
    dev.upload_index(12, 3, c["idx"].lookup, c["idx"].occ[:c["idx"].n_occ])
    return dev


def _stage(dev, c, slot, quals_on_host=False):
    batch = fo.ReadBatch(c["reads"])
    q = np.frombuffer("".join(c["quals"]).encode("latin-1"), np.uint8)
    dev.stage_reads(batch.bases, batch.off, slot=slot)
    dev.stage_text(q, c["rnames"], slot=slot, quals_on_host=quals_on_host)
    dev.map_staged(e=c["e"], slot=slot)
    return (q, batch.off) if quals_on_host else (None, None)


def _sam(dev, c, slot, quals_on_host=False):
    q, off = _stage(dev, c, slot, quals_on_host)
    return dev.fetch_sam(slot=slot, quals=q, offsets=off)


def _same(got, want):
    if got != want:  # (the first difference, not two texts of megabytes)
        g, w = got.split(b"\n"), want.split(b"\n")
        k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        raise AssertionError("line %d of %d / %d:\n%r\n%r" % (k, len(g), len(w), g[k:k + 1], w[k:k + 1]))


@pytest.mark.parametrize("case", SINGLE_CASES, ids=lambda x: "seed%d" % x[0])
def test_single_end_equals_the_model(case):
    c = single_case(*case)
    check_single_case(c)
    n, res = len(c["reads"]), c["res"]
    n_unm = len(um.unmapped_reads(res, n))
    dev = _device(c)
    try:
        off = _sam(dev, c, 0)[0]
        for mapq in (False, True):
            dev.set_mapq(mapq, slot=1)
            dev.set_unmapped(True, slot=1)
            want = um.single_end(res, c["names"], c["reads"], c["rnames"], c["quals"], e=c["e"] if mapq else None)
            on, n_records, _, stats = _sam(dev, c, 1)
            _same(on, want)
            assert n_records == int(res.rec_off[-1]) and dev.unmapped_count(slot=1) == n_unm == n - int(stats[1])
            # the qualities on the host: an unmapped read's field is sized, left open and filled like any other
            _same(_sam(dev, c, 1, quals_on_host=True)[0], want)
            assert dev.unmapped_count(slot=1) == n_unm
            # BAM at both levels: the model's encoding of the device's own text
            _stage(dev, c, 1)
            assert _bam_vs_sam(dev, 1, [x.encode() for x in c["names"]], n_sam=True) == on
            assert dev.unmapped_count(slot=1) == n_unm
            if not mapq:  # minus its FLAG & 4 lines the text is the default text
                rest, removed = um.without_unmapped(on)
                assert rest == off and removed == n_unm
        # off again: the bytes of a slot that never had it
        dev.set_mapq(False, slot=1)
        dev.set_unmapped(False, slot=1)
        assert _sam(dev, c, 1)[0] == off and dev.unmapped_count(slot=1) == 0
    finally:
        dev.close()


@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda x: "seed%d" % x[0])
def test_pairs_equal_the_model(case):
    c = pair_case(*case)
    check_pair_case(c)
    n, res, withr = c["n"], c["res"], c["withr"]
    after = withr if withr is not None else res
    n_unm = len(um.unmapped_reads(after, 2 * n))
    dev = _device(c)
    try:
        for slot in (0, 1):
            dev.set_pairs(I, X, slot=slot)
            if c["E"] is not None:
                dev.set_rescue(c["E"], slot=slot)
        off = _sam(dev, c, 0)[0]
        for mapq in (False, True):
            dev.set_mapq(mapq, slot=1)
            dev.set_unmapped(True, slot=1)
            want = um.paired(res, n, c["names"], c["reads"], c["rnames"], c["quals"], I, X, res=withr, rescued=set(c["kept"]),
                             e=c["e"] if mapq else None)
            on, n_records, _, stats = _sam(dev, c, 1)
            _same(on, want)
            n_resc = dev.rescue_count(slot=1) if c["E"] is not None else 0
            assert n_resc == len(c["kept"])
            assert dev.unmapped_count(slot=1) == n_unm == 2 * n - int(stats[1]) - n_resc
            _same(_sam(dev, c, 1, quals_on_host=True)[0], want)
            _stage(dev, c, 1)
            assert _bam_vs_sam(dev, 1, [x.encode() for x in c["names"]], n_sam=True) == on
            if not mapq:  # ... and with * 0 back in the mate columns of the 0x8 lines
                rest, removed = um.without_unmapped(on, True)
                assert rest == off and removed == n_unm
        dev.set_mapq(False, slot=1)
        dev.set_unmapped(False, slot=1)
        assert _sam(dev, c, 1)[0] == off and dev.unmapped_count(slot=1) == 0
        # fem_batch_pairs is what it is without the switch (output text only)
        dev.set_unmapped(True, slot=0)
        _stage(dev, c, 0)
        assert int(np.count_nonzero(dev.fetch_pairs(slot=0).mate_tid == 0xFFFFFFFF)) == sum(
            1 for l in off.splitlines() if int(l.split(b"\t")[1]) & 8)
    finally:
        dev.close()


def test_nothing_maps_and_an_empty_batch():
    rng = np.random.default_rng(120)
    c = dict(seqs=[util.rand_seq(rng, 5000)], names=["tiny"], e=3)
    c["reads"] = [util.rand_seq(rng, int(rng.integers(30, 160))) for _ in range(700)]
    c["rnames"] = ["x%d" % i for i in range(700)]
    c["quals"] = _quals(c["reads"])
    ref = fo.Reference(c["seqs"])
    c["idx"] = fo.OracleIndex(ref)
    res = fo.map_reads(ref, c["idx"], fo.ReadBatch(c["reads"]), e=3, threads=4)
    assert int(res.rec_off[-1]) == 0
    dev = _device(c)
    try:
        dev.set_unmapped(True)
        text, n_records, _, _ = _sam(dev, c, 0)
        _same(text, um.single_end(res, c["names"], c["reads"], c["rnames"], c["quals"]))
        assert n_records == 0 and dev.unmapped_count() == 700
        _stage(dev, c, 0)
        _bam_vs_sam(dev, 0, [b"tiny"], n_sam=True)
        dev.set_pairs(I, X)
        _same(_sam(dev, c, 0)[0], um.paired(res, 350, c["names"], c["reads"], c["rnames"], c["quals"]))
        empty = dict(c, reads=[], rnames=[], quals=[])
        assert _sam(dev, empty, 0)[0] == b"" and dev.unmapped_count() == 0
    finally:
        dev.close()


def test_kernel_time_ids():
    rng = np.random.default_rng(8)
    c = dict(seqs=[util.rand_seq(rng, 100_000)], names=["c"], e=3)
    c["reads"] = util.make_reads(rng, c["seqs"], 300, 100, 3)[:280] + [util.rand_seq(rng, 100) for _ in range(20)]
    c["rnames"] = ["r%d" % i for i in range(300)]
    c["quals"] = ["I" * 100] * 300
    c["idx"] = fo.OracleIndex(fo.Reference(c["seqs"]))
    dev = _device(c)
    try:
        dev.set_timing(True)
        for on, pairs in ((False, False), (True, False), (True, True), (False, True)):
            dev.set_unmapped(on)
            dev.set_pairs(I, X) if pairs else dev.set_pairs(None)
            dev.reset_timing()
            for k in range(2):
                _stage(dev, c, 0)
                dev.fetch_sam()
                _stage(dev, c, 0)
                dev.fetch_bam(level=0)
            assert dev.kernel_time(14)[1] == (4 if on else 0)
            assert dev.kernel_time(14)[0] > 0 or not on
            assert all(dev.kernel_time(i)[1] == 4 for i in (3, 4, 5))
            assert dev.kernel_time(7)[1] == 2 and dev.kernel_time(11)[1] == 2 and dev.kernel_time(13)[1] == 0
            assert dev.kernel_time(9)[1] == (4 if pairs else 0)
    finally:
        dev.close()


# ---- FEM map --unmapped ----

def _map(*args, env=None):
    e = dict(os.environ, **(env or {}))
    return subprocess.run([FEM, "map"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=e)


def _counter(err, what):
    return [int(l.rsplit(": ", 1)[1]) for l in err.decode().splitlines() if l.startswith("The number of " + what + ":")]


def test_cli(tmp_path):
    rng = np.random.default_rng(131)
    seqs, _ = _reference(rng, True)
    names = ["s%d" % i for i in range(len(seqs))]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = str(tmp_path / "ref.idx")
    subprocess.run([FEM, "index", "12", "3", str(fa), idx_path], check=True, capture_output=True, timeout=600)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, len(s)) for nm, s in zip(names, seqs)).encode()
    n, e, E = 2000, 3, 6
    se = util.make_reads(rng, seqs, n, 100, e)
    x1, x2 = make_rescue_pairs(rng, seqs, n, 100, 100, e, E, X, frac=0.2)
    for i in range(n):
        u = rng.random()
        if u < 0.25:
            se[i] = util.rand_seq(rng, 100)
        if u < 0.1 or u >= 0.92:
            x1[i] = util.rand_seq(rng, 100)
        if u >= 0.84:
            x2[i] = util.rand_seq(rng, 100)
    q = ["".join(chr(33 + (7 * i + j) % 40) for j in range(100)) for i in range(n)]
    rn = ["r%d" % i for i in range(n)]
    files = {}
    for key, reads, suffix in (("se", se, ""), ("x1", x1, "/1"), ("x2", x2, "/2")):
        files[key] = tmp_path / (key + ".fq")
        _write_fastq(files[key], reads, [x + suffix for x in rn], q, False)
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    common = ["-e", str(e), "-t", "4", "--ref", str(fa), "--index", idx_path, "--batch", "700", "--unmapped"]
    # single-end: SAM, BAM, the qualities on the host, two workers
    res = fo.map_reads(ref, idx, fo.ReadBatch(se), e=e, threads=8)
    want = header + um.single_end(res, names, se, rn, q)
    n_unm = len(um.unmapped_reads(res, n))
    assert 0.05 * n <= n_unm <= 0.95 * n
    out = str(tmp_path / "se.sam")
    r = _map(*(common + ["--read1", str(files["se"]), "-o", out]))
    assert r.returncode == 0, r.stderr.decode()
    _same(open(out, "rb").read(), want)
    assert _counter(r.stderr, "unmapped reads") == [n_unm] and _counter(r.stderr, "mapped read") == [n - n_unm]
    err = r.stderr.decode().splitlines()  # (behind the other counters, before Time)
    k = next(i for i, l in enumerate(err) if l.startswith("The number of unmapped reads"))
    assert err[k - 1].startswith("The number of mapping:") and err[k + 1].startswith("Time:")
    r = _map(*(common + ["--read1", str(files["se"]), "-o", out + ".bam", "--bam"]))
    assert r.returncode == 0, r.stderr.decode()
    _same(_decode_bam_file(out + ".bam"), want)
    assert _counter(r.stderr, "unmapped reads") == [n_unm]
    r = _map(*(common + ["--read1", str(files["se"]), "-o", out + ".hq"]), env={"FEM_HOST_QUALS": "1"})
    assert r.returncode == 0, r.stderr.decode()
    _same(open(out + ".hq", "rb").read(), want)
    r = _map(*(common + ["--read1", str(files["se"]), "-o", out + ".g2", "--gpus", "2"]), env={"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"})
    assert r.returncode == 0, r.stderr.decode()
    assert sorted(open(out + ".g2", "rb").read().splitlines()) == sorted(want.splitlines())
    assert _counter(r.stderr, "unmapped reads") == [n_unm]
    # without the switch: no such line on stderr
    r = _map(*([x for x in common if x != "--unmapped"] + ["--read1", str(files["se"]), "-o", out + ".off"]))
    assert r.returncode == 0 and not _counter(r.stderr, "unmapped reads")
    assert open(out + ".off", "rb").read() == header + um.without_unmapped(want[len(header):])[0]
    # read pairs with rescue and MAPQ: SAM, BAM (level 0 too), two workers
    reads = x1 + x2
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    withr, kept, _ = rm.rescue(res, n, reads, seqs, E, I, X)
    assert len(kept) >= 20 and min(um.pair_classes(withr, n)) >= 20
    want = header + um.paired(res, n, names, reads, rn + rn, q + q, I, X, res=withr, rescued=set(kept), e=e)
    n_unm = len(um.unmapped_reads(withr, 2 * n))
    pargs = common + ["--read1", str(files["x1"]), "--read2", str(files["x2"]), "--rescue", str(E), "--mapq"]
    out = str(tmp_path / "pe.sam")
    r = _map(*(pargs + ["-o", out]))
    assert r.returncode == 0, r.stderr.decode()
    _same(open(out, "rb").read(), want)
    assert _counter(r.stderr, "unmapped reads") == [n_unm] and _counter(r.stderr, "rescued mates") == [len(kept)]
    for flag in ("--bam", "--bam=0"):
        r = _map(*(pargs + ["-o", out + ".bam", flag]))
        assert r.returncode == 0, r.stderr.decode()
        _same(_decode_bam_file(out + ".bam"), want)
    r = _map(*(pargs + ["-o", out + ".g2", "--gpus", "2"]), env={"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"})
    assert r.returncode == 0, r.stderr.decode()
    assert sorted(open(out + ".g2", "rb").read().splitlines()) == sorted(want.splitlines())
    # the host paths have no such lines: refused
    for v in ("FEM_HOST_TAIL", "FEM_HOST_FORMAT"):
        r = _map(*(common + ["--read1", str(files["se"]), "-o", out + ".no"]), env={v: "1"})
        assert r.returncode != 0 and ("--unmapped is not supported with %s=1" % v) in r.stderr.decode()


def test_cli_nothing_maps(tmp_path):
    rng = np.random.default_rng(132)
    seq = util.rand_seq(rng, 3000)
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b">tiny\n" + seq + b"\n")
    idx_path = str(tmp_path / "ref.idx")
    subprocess.run([FEM, "index", "12", "3", str(fa), idx_path], check=True, capture_output=True, timeout=600)
    n = 5000
    reads = [util.rand_seq(rng, 150) for _ in range(n)]
    q = ["".join(chr(33 + (5 * i + j) % 41) for j in range(150)) for i in range(n)]
    rn = ["a_rather_long_read_name_%d" % i for i in range(n)]
    fq = tmp_path / "r.fq"
    _write_fastq(fq, reads, rn, q, False)
    for extra in ([], ["--bam"]):
        out = str(tmp_path / "out")
        r = _map("-e", "3", "-t", "4", "--ref", str(fa), "--index", idx_path, "--read1", str(fq), "-o", out, "--unmapped", *extra)
        assert r.returncode == 0, r.stderr.decode()
        text = _decode_bam_file(out) if extra else open(out, "rb").read()
        want = b"@SQ\tSN:tiny\tLN:3000\n" + b"".join(
            b"\t".join([a.encode(), b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b, c.encode()]) + b"\n" for a, b, c in zip(rn, reads, q))
        _same(text, want)
        assert _counter(r.stderr, "unmapped reads") == [n] and _counter(r.stderr, "mapping") == [0]
