"""The line filter on the device (fem_dev_set_report: report_kernel and the kUnm instances of the text and BAM record kernels,
fem_tail.hip) against the plain-Python rule of tests/report_model.py, applied to the expected text of the other models on the
oracle's records and to the device's own unfiltered text, on the cases of tests/cases.py.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import report_model as rp
from tests import rescue_model as rm
from tests import unmapped_model as um
from tests import util
from tests.cases import I, X, make_rescue_pairs, quals, write_fastq
from tests.cases import REPORT_PAIR_CASES as PAIR_CASES, REPORT_SINGLE_CASES as SINGLE_CASES
from tests.cases import check_report_pair_case as check_pair_case, check_report_single_case as check_single_case
from tests.cases import report_pair_case as pair_case, report_single_case as single_case, report_want
from tests.harness import bam_vs_sam, build_index, counter, decode_bam_file, fetch_sam, open_device, run_fem, same_text
from tests.harness import set_line_filter, stage_and_map

pytestmark = pytest.mark.gpu

# (S, N); None: off
FILTERS = [(0, None), (None, 1), (1, 3), (None, 33), (2, 64), (15, 2 ** 31 - 1)]


def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _stage(dev, c, slot, quals_on_host=False):
    return stage_and_map(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, quals_on_host)


def _sam(dev, c, slot, quals_on_host=False):
    return fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, quals_on_host)


def _check_filter(c, case, paired, strata, max_hits):
    n_lines_all = int((c["withr"] if paired and c["withr"] is not None else c["res"]).rec_off[-1])
    dev = _device(c)
    try:
        if paired:
            dev.set_pairs(I, X, slot=1)
            if c["E"] is not None:
                dev.set_rescue(c["E"], slot=1)
        ref_names = [x.encode() for x in c["names"]]
        for mapq in (False, True):
            for unmapped in (False, True):
                model = report_want(case, paired, mapq, unmapped)
                want, dropped = rp.apply(model, strata, max_hits)
                set_line_filter(dev, 1, mapq, unmapped, None, None)
                plain = _sam(dev, c, 1)[0]
                same_text(plain, model)
                assert dev.filtered_count(slot=1) == 0
                set_line_filter(dev, 1, mapq, unmapped, strata, max_hits)
                got, n_records, _, _ = _sam(dev, c, 1)
                same_text(got, want)
                same_text(got, rp.apply(plain, strata, max_hits)[0])
                if (strata, max_hits) == (15, 2 ** 31 - 1):
                    assert got == plain and dropped == 0
                else:
                    assert dropped > 0
                assert dev.filtered_count(slot=1) == dropped
                n_resc = dev.rescue_count(slot=1) if paired and c["E"] is not None else 0
                assert n_records == int(c["res"].rec_off[-1]) - dropped and n_records + n_resc == n_lines_all - dropped
                assert got.count(b"\n") == n_records + n_resc + dev.unmapped_count(slot=1)
                # BAM at both levels: the model's encoding of the device's own filtered text
                assert bam_vs_sam(dev, 1, ref_names, n_sam=True) == got
                assert dev.filtered_count(slot=1) == dropped
                # the qualities on the host: qual_at still finds every primary line's field
                same_text(_sam(dev, c, 1, quals_on_host=True)[0], want)
                assert dev.filtered_count(slot=1) == dropped
    finally:
        dev.close()


def _id(x):
    return "S%s_N%s" % tuple("off" if v is None else v for v in x)


@pytest.mark.parametrize("flt", FILTERS, ids=_id)
@pytest.mark.parametrize("case", SINGLE_CASES, ids=lambda x: "seed%d" % x[0])
def test_single_end_equals_the_model(case, flt):
    c = single_case(*case)
    check_single_case(c)
    _check_filter(c, case, False, *flt)


@pytest.mark.parametrize("flt", FILTERS, ids=_id)
@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda x: "seed%d" % x[0])
def test_pairs_equal_the_model(case, flt):
    c = pair_case(*case)
    check_pair_case(c)
    _check_filter(c, case, True, *flt)


def test_off_again_and_invalid_parameters():
    from fem_amd import FemError
    case = SINGLE_CASES[0]
    c = single_case(*case)
    dev = _device(c)
    try:
        off = _sam(dev, c, 0)[0]
        dev.set_report(0, 1, slot=1)
        got = _sam(dev, c, 1)[0]
        assert got == rp.apply(off, 0, 1)[0] and dev.filtered_count(slot=1) == off.count(b"\n") - got.count(b"\n") > 0
        dev.set_report(None, slot=1)
        assert _sam(dev, c, 1)[0] == off and dev.filtered_count(slot=1) == 0
        dev.set_report(max_hits=2, slot=1)
        assert _sam(dev, c, 1)[0] == rp.apply(off, None, 2)[0]
        for bad in (dict(strata=16), dict(strata=-2), dict(max_hits=0), dict(max_hits=-3), dict(max_hits=2 ** 31), dict(strata=0, max_hits=0)):
            with pytest.raises(FemError):
                dev.set_report(slot=1, **bad)
        assert _sam(dev, c, 1)[0] == rp.apply(off, None, 2)[0]  # (a refused call changes nothing)
        # the records and the pairs are not filtered
        _stage(dev, c, 1)
        assert dev.fetch_records(slot=1).n_records == int(c["res"].rec_off[-1])
    finally:
        dev.close()


def test_nothing_maps_and_an_empty_batch():
    rng = np.random.default_rng(220)
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
        dev.set_report(0, 1)
        assert _sam(dev, c, 0)[:2] == (b"", 0) and dev.filtered_count() == 0
        dev.set_unmapped(True)
        text, n_records, _, _ = _sam(dev, c, 0)
        same_text(text, um.single_end(res, c["names"], c["reads"], c["rnames"], c["quals"]))
        assert n_records == 0 and dev.unmapped_count() == 700 and dev.filtered_count() == 0
        _stage(dev, c, 0)
        bam_vs_sam(dev, 0, [b"tiny"], n_sam=True)
        dev.set_pairs(I, X)
        same_text(_sam(dev, c, 0)[0], um.paired(res, 350, c["names"], c["reads"], c["rnames"], c["quals"]))
        dev.set_unmapped(False)
        assert _sam(dev, c, 0)[0] == b""
        for unmapped in (False, True):
            dev.set_unmapped(unmapped)
            empty = dict(c, reads=[], rnames=[], quals=[])
            assert _sam(dev, empty, 0)[0] == b"" and dev.unmapped_count() == 0 and dev.filtered_count() == 0
    finally:
        dev.close()


def test_kernel_time_ids():
    rng = np.random.default_rng(9)
    c = dict(seqs=[util.rand_seq(rng, 100_000)], names=["c"], e=3)
    c["reads"] = util.make_reads(rng, c["seqs"], 300, 100, 3)[:280] + [util.rand_seq(rng, 100) for _ in range(20)]
    c["rnames"] = ["r%d" % i for i in range(300)]
    c["quals"] = ["I" * 100] * 300
    c["idx"] = fo.OracleIndex(fo.Reference(c["seqs"]))
    dev = _device(c)
    try:
        dev.set_timing(True)
        for flt, unmapped, pairs in ((None, False, False), ((0, None), False, False), ((None, 2), True, False), ((1, 2), True, True),
                                     (None, True, True), ((0, 1), False, True)):
            dev.set_report(*(flt or (None, None)))
            dev.set_unmapped(unmapped)
            dev.set_pairs(I, X) if pairs else dev.set_pairs(None)
            dev.reset_timing()
            for k in range(2):
                _stage(dev, c, 0)
                dev.fetch_sam()
                _stage(dev, c, 0)
                dev.fetch_bam(level=0)
            assert dev.kernel_time(15)[1] == (4 if flt else 0)
            assert dev.kernel_time(15)[0] > 0 or not flt
            assert dev.kernel_time(14)[1] == (4 if unmapped and not flt else 0)  # (the filter's line index is the unmapped reads' too)
            assert all(dev.kernel_time(i)[1] == 4 for i in (3, 4, 5))
            assert dev.kernel_time(7)[1] == 2 and dev.kernel_time(11)[1] == 2 and dev.kernel_time(13)[1] == 0
    finally:
        dev.close()


# ---- FEM map --strata / --max-hits ----

def test_cli(tmp_path):
    rng = np.random.default_rng(231)
    seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200) + [util.rand_seq(rng, 120_000)]
    names = ["s%d" % i for i in range(len(seqs))]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = str(tmp_path / "ref.idx")
    build_index(fa, idx_path)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, len(s)) for nm, s in zip(names, seqs)).encode()
    n, e, E, S, N = 1500, 3, 8, 0, 2
    se = util.make_reads(rng, seqs, n, 100, e)
    x1, x2 = make_rescue_pairs(rng, seqs, n, 100, 100, e, E, X, frac=0.2)
    for i in range(n):
        u = rng.random()
        if u < 0.2:
            se[i] = util.rand_seq(rng, 100)
        if u < 0.1:
            x1[i] = util.rand_seq(rng, 100)
    q = ["".join(chr(33 + (7 * i + j) % 40) for j in range(100)) for i in range(n)]
    rn = ["r%d" % i for i in range(n)]
    files = {}
    for key, reads, suffix in (("se", se, ""), ("x1", x1, "/1"), ("x2", x2, "/2")):
        files[key] = tmp_path / (key + ".fq")
        write_fastq(files[key], reads, [x + suffix for x in rn], q, False)
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    share = {"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"}
    common = ["-e", str(e), "-t", "4", "--ref", str(fa), "--index", idx_path, "--batch", "400", "--gpus", "2", "--strata", str(S),
              "--max-hits", str(N)]
    # single-end
    res = fo.map_reads(ref, idx, fo.ReadBatch(se), e=e, threads=8)
    want, dropped = rp.single_end(res, names, se, rn, q, unmapped=False, strata=S, max_hits=N)
    assert dropped > n
    # read pairs with rescue, MAPQ and the unmapped reads' lines
    reads = x1 + x2
    resp = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    withr, kept, _ = rm.rescue(resp, n, reads, seqs, E, I, X)
    wantp, droppedp = rp.paired(resp, n, names, reads, rn + rn, q + q, I, X, res=withr, rescued=set(kept), e=e, strata=S, max_hits=N)
    assert len(kept) >= 20 and droppedp > n
    pargs = ["--read1", str(files["x1"]), "--read2", str(files["x2"]), "--rescue", str(E), "--mapq", "--unmapped"]
    for args, text, count in ((["--read1", str(files["se"])], want, dropped), (pargs, wantp, droppedp)):
        for bam in (False, True):
            out = str(tmp_path / "out")
            r = run_fem("map", *(common + args + ["-o", out] + (["--bam"] if bam else [])), env=share)
            assert r.returncode == 0, r.stderr.decode()
            got = decode_bam_file(out) if bam else open(out, "rb").read()
            assert got.startswith(header)
            # (two workers: the batches' texts arrive in any order; a batch is whole reads / whole pairs)
            assert sorted(got[len(header):].splitlines()) == sorted(text.splitlines())
            assert rp.apply(got[len(header):], S, N) == (got[len(header):], 0)
            assert counter(r.stderr, "filtered lines") == [count]
            err = r.stderr.decode().splitlines()
            k = next(i for i, l in enumerate(err) if l.startswith("The number of filtered lines"))
            assert err[k + 1].startswith("Time:")  # (behind the other counters)
    # without the switches: no such line on stderr
    r = run_fem("map", "-e", str(e), "-t", "4", "--ref", str(fa), "--index", idx_path, "--read1", str(files["se"]), "-o", str(tmp_path / "off"))
    assert r.returncode == 0 and not counter(r.stderr, "filtered lines")
