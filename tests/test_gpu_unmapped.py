"""Lines for unmapped reads on the device (fem_dev_set_unmapped: the line index kernels and the kUnm instances of the text and
BAM record kernels, fem_tail.hip) against the plain-Python rule of tests/unmapped_model.py on the oracle's records, and against
the device's own default output, on the cases of tests/cases.py.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import rescue_model as rm
from tests import unmapped_model as um
from tests import util
from tests.cases import I, X, make_rescue_pairs, quals, reference, write_fastq
from tests.cases import UNMAPPED_PAIR_CASES as PAIR_CASES, UNMAPPED_SINGLE_CASES as SINGLE_CASES
from tests.cases import check_unmapped_pair_case as check_pair_case, check_unmapped_single_case as check_single_case
from tests.cases import unmapped_pair_case as pair_case, unmapped_single_case as single_case
from tests.harness import bam_vs_sam, build_index, counter, decode_bam_file, fetch_sam, open_device, run_fem, same_text, stage_and_map

pytestmark = pytest.mark.gpu


def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _stage(dev, c, slot, quals_on_host=False):
    return stage_and_map(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, quals_on_host)


def _sam(dev, c, slot, quals_on_host=False):
    return fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, quals_on_host)


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
            same_text(on, want)
            assert n_records == int(res.rec_off[-1]) and dev.unmapped_count(slot=1) == n_unm == n - int(stats[1])
            # the qualities on the host: an unmapped read's field is sized, left open and filled like any other
            same_text(_sam(dev, c, 1, quals_on_host=True)[0], want)
            assert dev.unmapped_count(slot=1) == n_unm
            # BAM at both levels: the model's encoding of the device's own text
            _stage(dev, c, 1)
            assert bam_vs_sam(dev, 1, [x.encode() for x in c["names"]], n_sam=True) == on
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
            same_text(on, want)
            n_resc = dev.rescue_count(slot=1) if c["E"] is not None else 0
            assert n_resc == len(c["kept"])
            assert dev.unmapped_count(slot=1) == n_unm == 2 * n - int(stats[1]) - n_resc
            same_text(_sam(dev, c, 1, quals_on_host=True)[0], want)
            _stage(dev, c, 1)
            assert bam_vs_sam(dev, 1, [x.encode() for x in c["names"]], n_sam=True) == on
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
    c["quals"] = quals(c["reads"])
    ref = fo.Reference(c["seqs"])
    c["idx"] = fo.OracleIndex(ref)
    res = fo.map_reads(ref, c["idx"], fo.ReadBatch(c["reads"]), e=3, threads=4)
    assert int(res.rec_off[-1]) == 0
    dev = _device(c)
    try:
        dev.set_unmapped(True)
        text, n_records, _, _ = _sam(dev, c, 0)
        same_text(text, um.single_end(res, c["names"], c["reads"], c["rnames"], c["quals"]))
        assert n_records == 0 and dev.unmapped_count() == 700
        _stage(dev, c, 0)
        bam_vs_sam(dev, 0, [b"tiny"], n_sam=True)
        dev.set_pairs(I, X)
        same_text(_sam(dev, c, 0)[0], um.paired(res, 350, c["names"], c["reads"], c["rnames"], c["quals"]))
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
    return run_fem("map", *args, env=env)


def test_cli(tmp_path):
    rng = np.random.default_rng(131)
    seqs, _ = reference(rng, True)
    names = ["s%d" % i for i in range(len(seqs))]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = str(tmp_path / "ref.idx")
    build_index(fa, idx_path)
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
        write_fastq(files[key], reads, [x + suffix for x in rn], q, False)
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
    same_text(open(out, "rb").read(), want)
    assert counter(r.stderr, "unmapped reads") == [n_unm] and counter(r.stderr, "mapped read") == [n - n_unm]
    err = r.stderr.decode().splitlines()  # (behind the other counters, before Time)
    k = next(i for i, l in enumerate(err) if l.startswith("The number of unmapped reads"))
    assert err[k - 1].startswith("The number of mapping:") and err[k + 1].startswith("Time:")
    r = _map(*(common + ["--read1", str(files["se"]), "-o", out + ".bam", "--bam"]))
    assert r.returncode == 0, r.stderr.decode()
    same_text(decode_bam_file(out + ".bam"), want)
    assert counter(r.stderr, "unmapped reads") == [n_unm]
    r = _map(*(common + ["--read1", str(files["se"]), "-o", out + ".hq"]), env={"FEM_HOST_QUALS": "1"})
    assert r.returncode == 0, r.stderr.decode()
    same_text(open(out + ".hq", "rb").read(), want)
    r = _map(*(common + ["--read1", str(files["se"]), "-o", out + ".g2", "--gpus", "2"]), env={"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"})
    assert r.returncode == 0, r.stderr.decode()
    assert sorted(open(out + ".g2", "rb").read().splitlines()) == sorted(want.splitlines())
    assert counter(r.stderr, "unmapped reads") == [n_unm]
    # without the switch: no such line on stderr
    r = _map(*([x for x in common if x != "--unmapped"] + ["--read1", str(files["se"]), "-o", out + ".off"]))
    assert r.returncode == 0 and not counter(r.stderr, "unmapped reads")
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
    same_text(open(out, "rb").read(), want)
    assert counter(r.stderr, "unmapped reads") == [n_unm] and counter(r.stderr, "rescued mates") == [len(kept)]
    for flag in ("--bam", "--bam=0"):
        r = _map(*(pargs + ["-o", out + ".bam", flag]))
        assert r.returncode == 0, r.stderr.decode()
        same_text(decode_bam_file(out + ".bam"), want)
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
    build_index(fa, idx_path)
    n = 5000
    reads = [util.rand_seq(rng, 150) for _ in range(n)]
    q = ["".join(chr(33 + (5 * i + j) % 41) for j in range(150)) for i in range(n)]
    rn = ["a_rather_long_read_name_%d" % i for i in range(n)]
    fq = tmp_path / "r.fq"
    write_fastq(fq, reads, rn, q, False)
    for extra in ([], ["--bam"]):
        out = str(tmp_path / "out")
        r = _map("-e", "3", "-t", "4", "--ref", str(fa), "--index", idx_path, "--read1", str(fq), "-o", out, "--unmapped", *extra)
        assert r.returncode == 0, r.stderr.decode()
        text = decode_bam_file(out) if extra else open(out, "rb").read()
        want = b"@SQ\tSN:tiny\tLN:3000\n" + b"".join(
            b"\t".join([a.encode(), b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b, c.encode()]) + b"\n" for a, b, c in zip(rn, reads, q))
        same_text(text, want)
        assert counter(r.stderr, "unmapped reads") == [n] and counter(r.stderr, "mapping") == [0]
