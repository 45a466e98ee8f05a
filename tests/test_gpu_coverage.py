"""The coverage track on the device (fem_dev_set_coverage: coverage_kernel behind the line index, fem_coverage.hip.h; the bins of
the handle) and FEM map --coverage: the bins the handle returns against the plain-Python rule of tests/coverage_model.py applied
to the SAM text fetched in the same test, under the options that decide the lines.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from fem_amd import host
from fem_amd.device import STAGE_COVERAGE, STAGE_TEXT, FemError, live_bytes
from tests import bam_model as bm
from tests import cases, util
from tests import coverage_model as m
from tests.cases import I, LINE_E, LINE_RESCUE_E, MAX_HITS, STRATA, X, line_options_case, make_pairs, make_rescue_pairs, write_fastq
from tests.harness import (build_index, counter, counters, decode_bam_file, fetch_sam, open_device, open_reference, pairing_on, run_fem,
                           same_text, stage_and_map)

pytestmark = pytest.mark.gpu

WINDOWS = (1, 7, 64, 1000)
SECOND = 50_017  # the second sequence's length: no multiple of any window above


def _lens(seqs):
    return [len(s) for s in seqs]


def _model(text, c, W, **kw):
    return m.bins(text, c["names"], _lens(c["seqs"]), W, **kw)


def _track(dev, c, W, all_hits=False, min_mapq=0, slot=0, bam=False):
    """The batch mapped once more into a zeroed track of window W -> (its SAM text, or the BAM records decoded; the bins)."""
    dev.set_coverage(W, all_hits, min_mapq)
    stage_and_map(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot)
    if bam:
        data = dev.fetch_bam(slot=slot, level=0)[0]
        payload = b"".join(x[0] for x in bm.parse_bgzf(data, eof=False)) if data else b""
        text = bm.bam_payload_to_sam(payload, [n.encode() for n in c["names"]])
    else:
        text = dev.fetch_sam(slot=slot)[0]
    got = dev.fetch_coverage()
    n_bins, off = dev.coverage_layout()
    assert n_bins == len(got) and off.tolist() == m.layout(_lens(c["seqs"]), W)
    return text, got


def _same_bins(got, want):
    assert got.dtype == np.uint64 and len(got) == len(want)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "bin %d of %d: got %d want %d (%d differ)" % (bad[0], len(got), got[bad[0]], want[bad[0]], len(bad))


def _spans(text, **kw):
    return sum(s for _, _, s in m.counting(text, **kw))


# ---- 1. single-end ----

@pytest.fixture(scope="module")
def single():
    rng, dev, ref, idx, seqs, names = open_reference(811, False, second=SECOND)
    dev.close()
    reads = util.make_reads(rng, seqs, 300, 100, 3)  # (both strands, 0 .. 3 edits: substitutions, insertions, deletions)
    # The ends of the sequences.  The mapper keeps a candidate only where the read's own start p has e <= p and p + L + e < n
    # (remove_out_ranged_candidates, reference src/filter.c:133-144; clip_to_reference of the oracle), so an unedited read that
    # touches base 0 or base n - 1 gets no line, and no line covers base n - 1.  The unedited reads at p = e and at
    # p = n - L - e - 1 are the nearest to the ends that the rule places for certain: they are the asserted case.
    for s in seqs:
        n = len(s)
        ends = [s[:100], s[-100:]]                                       # touch the ends: no line
        ends += [s[3:103], s[n - 104:n - 4]]                              # unedited, as near as the rule lets them
        reads += ends + [util.revcomp(x) for x in ends]
    reads += [util.rand_seq(rng, 100) for _ in range(8)]
    return dict(seqs=seqs, names=names, idx=idx, reads=reads, rnames=["s%d" % i for i in range(len(reads))], quals=cases.quals(reads), e=3)


def test_single_end(single):
    c = single
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        assert dev.stage_ms(STAGE_COVERAGE) < 0
        plain = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"])[0]
        assert dev.stage_ms(STAGE_COVERAGE) < 0 and dev.stage_ms(STAGE_TEXT) > 0  # off is off: the stage did not run
        for W in WINDOWS:
            text, got = _track(dev, c, W)
            assert text == plain  # the option never touches a line
            assert dev.stage_ms(STAGE_COVERAGE) >= 0
            assert int(got.sum()) == _spans(text) > 200 * 90  # (most of the 300 drawn reads map at e = 3)
            _same_bins(got, _model(text, c, W))
        cols = [l.split(b"\t") for l in plain.splitlines()]
        assert any(b"I" in f[5] for f in cols) and any(b"D" in f[5] for f in cols) and any(int(f[1]) & 16 for f in cols)
        # the ends of both sequences, on either strand: a counting line that starts within e bases of base 0 and one that ends
        # within e bases of base n - 1, the first base no line can cover
        for name, s in zip(c["names"], c["seqs"]):
            for rev in (0, 16):
                mine = [(int(f[3]) - 1, int(f[3]) - 1 + m.span(f[5])) for f in cols if f[2] == name.encode() and int(f[1]) & 16 == rev]
                assert any(p <= c["e"] for p, _ in mine) and any(q >= len(s) - c["e"] - 1 for _, q in mine), (name, rev)
        for W in (64, 1000):  # the last window of the second sequence has 33 and 17 bases
            text, got = _track(dev, c, W)
            want, off = _model(text, c, W), dev.coverage_layout()[1]
            for t in range(len(c["seqs"])):  # the first and the last bin of each sequence's range: covered, and the model's
                for k in (int(off[t]), int(off[t + 1]) - 1):
                    assert got[k] == want[k] > 0, (W, t, k)
    finally:
        dev.close()


# ---- 2. a repeat: many lines on the same few bins ----

@pytest.fixture(scope="module")
def repeat():
    rng = np.random.default_rng(812)
    L = 100
    seqs, names, units, _, _ = cases.report_reference(rng, L, copies=(130, 2))
    seqs, names = seqs[2:4], names[2:4]  # the random sequence and the one with the units
    (u130, _), (u2, _) = units
    reads = [u130[o:o + L] for o in rng.integers(0, 61, 150)] + [u2[o:o + L] for o in rng.integers(0, 61, 10)]
    reads += util.make_reads(rng, seqs[:1], 20, L, 0)
    return dict(seqs=seqs, names=names, idx=None, reads=reads, rnames=["h%d" % i for i in range(len(reads))], quals=cases.quals(reads), e=3)


@pytest.mark.parametrize("all_hits", [False, True], ids=["primary", "all_hits"])
def test_repeat(repeat, all_hits):
    c = repeat
    dev = open_device(c["seqs"], c["names"])[0]
    try:
        for W in (1, 1000):
            text, got = _track(dev, c, W, all_hits)
            n_lines = text.count(b"\n")
            assert n_lines >= 150 * 130
            assert int(got.sum()) == _spans(text, all_hits=all_hits) >= (n_lines if all_hits else 150) * 95
            _same_bins(got, _model(text, c, W, all_hits=all_hits))
            if W == 1000 and all_hits:  # the contention: thousands of lines into one bin
                assert int(got.max()) > 150 * 100
    finally:
        dev.close()


# ---- 3. pairs, both rescues, placed unmapped lines ----

def test_pairs_with_rescue():
    rng, dev, ref, idx, seqs, names = open_reference(813, False, second=SECOND)
    try:
        E = 8
        r1, r2 = make_rescue_pairs(rng, seqs, 150, 100, 100, 2, E, X, near_end=True)
        r1 += [util.rand_seq(rng, 100)] * 2  # a pair with one mate unmapped (placed at its mate), one with both
        r2 += [seqs[0][5000:5100], util.rand_seq(rng, 100)]
        n = len(r1)
        reads = r1 + r2
        c = dict(seqs=seqs, names=names, reads=reads, rnames=["p%d" % i for i in range(n)] * 2, quals=cases.quals(reads), e=2)
        pairing_on(dev, I, X, E)
        for W, all_hits in ((64, False), (1000, True)):
            text, got = _track(dev, c, W, all_hits)
            assert dev.rescue_count() > 0 and dev.unmapped_count() >= 2
            cols = [l.split(b"\t") for l in text.splitlines()]
            assert any(int(f[1]) & 4 and f[2] != b"*" for f in cols)  # a placed unmapped line: RNAME and POS, and no coverage
            _same_bins(got, _model(text, c, W, all_hits=all_hits))
            assert int(got.sum()) == _spans(text, all_hits=all_hits)
        dev.set_unmapped(False)
        text, got = _track(dev, c, 64)
        _same_bins(got, _model(text, c, 64))
    finally:
        dev.close()


# ---- 4. the options drawn together ----

def test_options_together():
    c = dict(line_options_case(), e=LINE_E)
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    W = 64
    try:
        pairing_on(dev, I, X, LINE_RESCUE_E)
        dev.set_tags(hits=True)
        dev.set_mate_tags(True)
        seen = set()
        for flt in (False, True):
            dev.set_report(strata=STRATA, max_hits=MAX_HITS) if flt else dev.set_report()
            for min_mapq in (0, 1, 30, 60):
                for all_hits in (False, True):
                    dev.set_xa(0)
                    plain, got = _track(dev, c, W, all_hits, min_mapq)
                    _same_bins(got, _model(plain, c, W, all_hits=all_hits, min_mapq=min_mapq))
                    dev.set_xa(2)  # small: some secondary lines fold, some stay lines
                    folded, got_xa = _track(dev, c, W, all_hits, min_mapq)
                    assert dev.xa_count() > 0
                    if not flt:  # (the filter's hit limit leaves a slot no more secondary lines than fold)
                        assert any(int(l.split(b"\t")[1]) & 0x100 for l in folded.splitlines())
                    _same_bins(got_xa, got)  # folding never changes the track
                    if min_mapq == 0:  # (an entry carries no MAPQ: the text with XA is a model's input at threshold 0 alone)
                        _same_bins(got_xa, _model(folded, c, W, all_hits=all_hits))
                    seen.add(got.tobytes())
            if flt:
                assert dev.filtered_count() > 0
        assert len(seen) >= 4  # the filter, the threshold and the mode each change what counts
    finally:
        dev.close()


# ---- 5. a trimmed batch ----

def test_trimmed_batch(single):
    c = single
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        dev.set_trim(trim5=9, trim3=6)
        text, got = _track(dev, c, 7)
        cigars = [l.split(b"\t")[5] for l in text.splitlines()]
        assert cigars and all(x.startswith((b"9S", b"6S")) and x.endswith(b"S") for x in cigars)
        assert int(got.sum()) == _spans(text) <= 85 * len(cigars) + 3 * len(cigars)  # the kept parts' spans (85 bases, +- indels)
        _same_bins(got, _model(text, c, 7))
    finally:
        dev.close()


# ---- 6. SAM and BAM ----

def test_bam_adds_what_sam_adds(single):
    c = single
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        text, got = _track(dev, c, 64)
        as_bam, got_bam = _track(dev, c, 64, bam=True)
        same_text(as_bam, text)
        _same_bins(got_bam, got)
        assert dev.stage_ms(STAGE_COVERAGE) >= 0
    finally:
        dev.close()


# ---- 7. accumulation ----

def test_accumulation(single):
    c = single
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    W = 64
    n = len(c["reads"])
    parts = [dict(c, reads=c["reads"][a:b], rnames=c["rnames"][a:b], quals=c["quals"][a:b]) for a, b in ((0, 120), (120, 121), (121, n))]
    try:
        dev.set_coverage(W)
        want = np.zeros(len(dev.fetch_coverage()), np.uint64)
        assert not dev.fetch_coverage().any()
        # three batches over two slots, both mapped before either is fetched, the second fetched first
        for p, slot in zip(parts[:2], (0, 1)):
            stage_and_map(dev, p["reads"], p["rnames"], p["quals"], p["e"], slot)
        texts = {1: dev.fetch_sam(slot=1, nowait=True)[0]}  # (_nowait, then _sam_wait)
        _same_bins(dev.fetch_coverage(), _model(texts[1], c, W))
        texts[0] = dev.fetch_sam(slot=0)[0]
        stage_and_map(dev, parts[2]["reads"], parts[2]["rnames"], parts[2]["quals"], c["e"], 0)
        texts[2] = dev.fetch_bam(slot=0, level=0) and dev.fetch_sam(slot=0)[0]  # the BAM fetch adds, the text behind it does not
        for t in texts.values():
            want += _model(t, c, W)
        _same_bins(dev.fetch_coverage(), want)
        assert b"".join(texts[k] for k in (0, 1, 2)) == fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 1)[0]
        want += _model(texts[0] + texts[1] + texts[2], c, W)  # (that was a fourth batch: the whole case once more)
        _same_bins(dev.fetch_coverage(), want)
        assert dev.fetch_sam(slot=1)[0] and dev.fetch_sam(slot=0)[0]  # further fetches of the same batches
        _same_bins(dev.fetch_coverage(), want)
        stage_and_map(dev, c["reads"], c["rnames"], c["quals"], c["e"], 0)
        assert len(dev.fetch_records(slot=0).flag) > 200  # mapped, but never fetched as text or BAM
        _same_bins(dev.fetch_coverage(), want)
        dev.reset_coverage()
        assert not dev.fetch_coverage().any()
        assert dev.fetch_sam(slot=0)[0]  # (the batch of the records fetch: its first text adds it)
        _same_bins(dev.fetch_coverage(), _model(texts[0] + texts[1] + texts[2], c, W))
    finally:
        dev.close()


# ---- 8. tiny batches ----

def test_tiny_batches(single):
    c = single
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    rng = np.random.default_rng(3)
    try:
        for unmapped in (False, True):
            dev.set_unmapped(unmapped)
            for reads in ([], [c["seqs"][1][1000:1100]], [util.rand_seq(rng, 100) for _ in range(70)]):
                p = dict(c, reads=reads, rnames=c["rnames"][:len(reads)], quals=cases.quals(reads))
                text, got = _track(dev, p, 7)
                assert text.count(b"\n") == (len(reads) if unmapped or len(reads) == 1 else 0)
                assert int(got.sum()) == (100 if len(reads) == 1 else 0)
                _same_bins(got, _model(text, c, 7))
    finally:
        dev.close()


# ---- 9. off is off, the refusals, the memory ----

def test_refusals_and_memory(single):
    c = single
    from fem_amd import Device
    dev = Device(0)
    try:
        with pytest.raises(FemError):
            dev.set_coverage(1000)  # no reference yet
        dev.set_coverage(None)      # off may always be asked for
    finally:
        dev.close()
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        with pytest.raises(FemError):
            dev.fetch_coverage()  # off
        with pytest.raises(FemError):
            dev.reset_coverage()
        before = live_bytes()
        dev.set_coverage(64, True, 30)
        n_bins = dev.coverage_layout()[0]
        assert live_bytes()[0] >= before[0] + 8 * n_bins
        for bad in ((0, 0, 0), (1_000_001, 0, 0), (64, 2, 0), (64, 0, 61), (64, 0, -1)):
            with pytest.raises(FemError):
                dev.set_coverage(*bad)
        assert dev.coverage_layout()[0] == n_bins  # a refused call leaves the setting as it was
        with pytest.raises(FemError):
            dev.fetch_coverage(cap=n_bins - 1)
        assert len(dev.fetch_coverage(cap=n_bins + 5)) == n_bins
        dev.set_coverage(None)
        assert live_bytes() == before
        with pytest.raises(FemError):
            dev.fetch_coverage()
        text = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"])[0]  # off again: a text as ever, no stage
        assert text and dev.stage_ms(STAGE_COVERAGE) < 0
        dev.set_coverage(1)
        opened = live_bytes()
    finally:
        dev.close()
    assert live_bytes()[0] < opened[0] - 8 * 250_000  # the track went with the handle


# ---- 10. FEM map --coverage ----

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("coverage")
    rng = np.random.default_rng(814)
    seqs, names = cases.reference(rng, True)
    fa = tmp / "ref.fa"
    fa.write_bytes(b"".join(b">%s desc\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    idx_path = str(tmp / "ref.idx")
    build_index(fa, idx_path)
    n = 400
    x1, x2 = make_pairs(rng, seqs, n, 100, 2)
    rn = ["m%d" % i for i in range(n)]
    p1, p2 = tmp / "x1.fq", tmp / "x2.fq"
    write_fastq(p1, x1, rn, cases.quals(x1), False)
    write_fastq(p2, x2, rn, cases.quals(x2), False)
    return dict(tmp=tmp, fa=str(fa), idx=idx_path, p1=str(p1), p2=str(p2), n=n, names=names, lens=_lens(seqs))


def _cli(files, *args, bam=False, env=None):
    out, cov = str(files["tmp"] / "out"), str(files["tmp"] / "cov.bed")
    common = ["-e", "2", "-t", "16", "--ref", files["fa"], "--index", files["idx"], "--read1", files["p1"], "--read2", files["p2"], "--rescue", "8",
              "--unmapped", "-o", out]
    r = run_fem("map", *(common + [a if a != "COV" else cov for a in args]), env=env)
    if r.returncode:
        return r, None, None
    got = decode_bam_file(out) if bam else open(out, "rb").read()
    sam = b"".join(l + b"\n" for l in got.splitlines() if not l.startswith(b"@"))
    return r, sam, (open(cov, "rb").read() if "COV" in args else None)


def _want_bed(files, sam, W, **kw):
    track = m.bins(sam, files["names"], files["lens"], W, **kw)
    path = str(files["tmp"] / "want.bed")
    total = host.coverage_write(path, files["names"], files["lens"], W, track)
    assert total == int(track.sum())
    return open(path, "rb").read(), total


def test_cli(files):
    plain, plain_sam, _ = _cli(files)
    assert plain.returncode == 0 and not counter(plain.stderr, "covered bases")
    for args, W, kw, bam in ((("--coverage", "COV"), 1000, {}, False),
                             (("--coverage", "COV", "--bam"), 1000, {}, True),
                             (("--coverage", "COV", "--coverage-window", "64", "--batch", "90"), 64, {}, False),
                             (("--coverage", "COV", "--coverage-window", "7", "--coverage-all"), 7, dict(all_hits=True), False)):
        r, sam, bed = _cli(files, *args, bam=bam)
        assert r.returncode == 0, r.stderr.decode()
        same_text(sam, plain_sam)  # the switch never touches a line
        want, total = _want_bed(files, sam, W, **kw)
        assert bed == want and total > 200 * 100
        assert counters(r.stderr)[:-1] == counters(plain.stderr) and counter(r.stderr, "covered bases") == [total]
        assert counters(r.stderr)[-1].startswith("The number of covered bases")  # behind the existing counter lines
    r, sam, bed = _cli(files, "--coverage", "COV", "--mapq", "--coverage-mapq", "30", "--xa=2", "--coverage-all")
    assert r.returncode == 0, r.stderr.decode()
    r0, sam0, _ = _cli(files, "--mapq")  # (the same lines without XA: an entry carries no MAPQ)
    assert r0.returncode == 0 and counter(r.stderr, "XA entries")[0] > 0
    want, total = _want_bed(files, sam0, 1000, all_hits=True, min_mapq=30)
    assert bed == want and 0 < total < _want_bed(files, sam0, 1000, all_hits=True)[1]


def test_cli_refusals(files):
    for args, env, word in ((("--coverage", "COV", "--coverage-mapq", "30"), None, b"--coverage-mapq needs --mapq"),
                            (("--coverage-window", "64"), None, b"need --coverage"),
                            (("--coverage-all",), None, b"need --coverage"),
                            (("--mapq", "--coverage-mapq", "30"), None, b"need --coverage"),
                            (("--coverage", "COV", "--coverage-window", "0"), None, b"Wrong coverage window"),
                            (("--coverage", "COV", "--coverage-window", "1000001"), None, b"Wrong coverage window"),
                            (("--coverage", "COV", "--mapq", "--coverage-mapq", "61"), None, b"Wrong coverage MAPQ"),
                            (("--coverage", "COV"), {"FEM_HOST_TAIL": "1"}, b"--coverage is not supported with FEM_HOST_TAIL=1"),
                            (("--coverage", "COV"), {"FEM_HOST_FORMAT": "1"}, b"--coverage is not supported with FEM_HOST_FORMAT=1")):
        # (without --unmapped, which the host switches refuse ahead of --coverage)
        argv = ["map", "-e", "2", "--ref", files["fa"], "--index", files["idx"], "--read1", files["p1"], "-o", str(files["tmp"] / "out_r")]
        r = run_fem(*(argv + [a if a != "COV" else str(files["tmp"] / "cov_r.bed") for a in args]), env=env)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)


def test_cli_two_gpus(files):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    r1, sam1, bed1 = _cli(files, "--coverage", "COV", "--batch", "90")
    r2, sam2, bed2 = _cli(files, "--coverage", "COV", "--batch", "90", "--gpus", "2")
    assert r1.returncode == 0 and r2.returncode == 0, r2.stderr.decode()
    assert bed2 == bed1 and counter(r2.stderr, "covered bases") == counter(r1.stderr, "covered bases")
