"""Secondary lines folded into XA:Z on the device (fem_dev_set_xa: xa_index_kernel and xa_write_kernel behind report_kernel's line
index, the kUnm instances of the text and BAM record kernels, fem_tail.hip) and FEM map --xa: the same handle's text with the option
off, then on, against the plain-Python rule of tests/xa_model.py; the BAM records decoded against the text; every count but the new
one unchanged.  Needs a GPU: -m gpu."""
import ctypes as C

import numpy as np
import pytest

from fem_amd.device import FemError
from tests import bam_model as bm
from tests import cases
from tests import xa_model as m
from tests.cases import I, LINE_E, LINE_RESCUE_E, MAX_HITS, RG, STRATA, X, line_options_case, make_pairs, write_fastq
from tests.harness import build_index, counter, counters, decode_bam_file, open_device, pairing_on, run_fem, same_text, stage_and_map

pytestmark = pytest.mark.gpu


def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _stage(dev, c, slot=0, packed=False, quals_on_host=False):
    return stage_and_map(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, quals_on_host, packed)


def _counts(dev, slot, paired):
    out = [dev.unmapped_count(slot=slot), dev.filtered_count(slot=slot)]
    if paired:
        out += [dev.pair_count(slot=slot), dev.rescue_count(slot=slot), dev.rescue_discordant_count(slot=slot)]
    return out


def _off(dev, c, slot=0, paired=False):
    """The staged batch's text with the option off -> what _on compares with."""
    dev.set_xa(0, slot=slot)
    text, n_records, n_asserted, stats = dev.fetch_sam(slot=slot)
    assert dev.xa_count(slot=slot) == 0
    return dict(text=text, n_records=n_records, n_asserted=n_asserted, stats=stats, counts=_counts(dev, slot, paired), paired=paired,
                names=[x.encode() for x in c["names"]])


def _on(dev, off, N, slot=0):
    """... and with it on at N: on == the rule applied to off, xa_count the model's count, n_records, n_asserted, the stats and every
    other count as off, the BAM records at both levels decode to on, nowait gives on -> (on, entries)."""
    want, n = m.apply(off["text"], N)
    dev.set_xa(N, slot=slot)
    on, n_records, n_asserted, stats = dev.fetch_sam(slot=slot)
    same_text(on, want)
    assert dev.xa_count(slot=slot) == n
    assert (n_records, n_asserted) == (off["n_records"], off["n_asserted"]) and np.array_equal(stats, off["stats"])
    assert _counts(dev, slot, off["paired"]) == off["counts"]
    for level in (0, 1):
        data, raw_len, _, n_rec_b, n_ass_b, stats_b = dev.fetch_bam(slot=slot, level=level)
        payload = b"".join(x[0] for x in bm.parse_bgzf(data, eof=False)) if data else b""
        assert raw_len == len(payload)
        same_text(bm.bam_payload_to_sam(payload, off["names"]), on)
        assert (n_rec_b, n_ass_b) == (off["n_records"], off["n_asserted"]) and np.array_equal(stats_b, off["stats"])
        assert dev.xa_count(slot=slot) == n and _counts(dev, slot, off["paired"]) == off["counts"]
    assert dev.fetch_sam(slot=slot, nowait=True)[0] == on
    return on, n


def _off_on(dev, c, N, slot=0, paired=False):
    off = _off(dev, c, slot, paired)
    on, n = _on(dev, off, N, slot)
    return off["text"], on, n


# ---- 1. slot sizes, single-end ----

@pytest.mark.parametrize("k", [0, 1])
def test_slot_sizes_single_end(k):
    case = cases.REPORT_SINGLE_CASES[k]
    c = cases.report_single_case(*case)
    cases.check_report_single_case(c)
    dev = _device(c)
    try:
        _stage(dev, c)
        off = _off(dev, c)
        if k == 0:  # the chain ends at the oracle
            same_text(off["text"], cases.report_want(case, False, False, False))
        folds = [len(s) - 1 for s in m.slots(off["text"])]
        assert set(m.FOLD_SIZES) <= set(folds) and max(folds) >= 199, sorted(set(folds))
        for N in m.N_LADDER:
            on, n = _on(dev, off, N)
            assert n == sum(min(f, N) for f in folds) > 0  # (entries of some twenty bytes: the budget stops nothing here)
            if N == 32:
                assert any(len(s) > 1 and m.xa_of(s[0]) for s in m.slots(on))  # a slot that keeps leftover secondary lines
        assert on.count(b"\n") == len(folds)  # N = all: a line per mapped read
    finally:
        dev.close()


# ---- 2. the byte budget on the device ----

def test_byte_budget_and_hit_tags():
    c = m.long_names(cases.report_single_case(*cases.REPORT_SINGLE_CASES[0]))
    dev = _device(c)
    try:
        dev.set_tags(hits=True)
        _stage(dev, c)
        off, on, n = _off_on(dev, c, m.ALL)
        stops = m.budget_stops(off)
        assert stops
        after = {s[0].split(b"\t", 1)[0]: s for s in m.slots(on)}
        for before, f in stops:
            got = after[before[0].split(b"\t", 1)[0]]
            value = m.xa_of(got[0])
            assert 1 <= f < len(before) - 1 and len(m.entries(got[0])) == f
            assert len(value) <= m.MAX_BYTES < len(value) + len(m.entry(before[1 + f]))
            assert got[1:] == before[1 + f:]  # its remaining lines follow l_0 unchanged
            assert m.tag(got[0], b"NH:i") == b"%d" % len(before) and m.tag(got[1], b"HI:i") == b"%d" % (f + 2)
        assert any(f > 64 for _, f in stops)  # ... inside a wave's walk of several steps
        # NH and HI of every surviving line are the off text's
        tags_off = {tuple(l.split(b"\t")[:4]): (m.tag(l, b"NH:i"), m.tag(l, b"HI:i")) for l in off.splitlines()}
        for l in on.splitlines():
            assert (m.tag(l, b"NH:i"), m.tag(l, b"HI:i")) == tags_off[tuple(l.split(b"\t")[:4])]
        _on(dev, _off(dev, c), 120)  # the entry limit beyond where the budget stops the large slot
    finally:
        dev.close()


# ---- 3. pairs ----

def _read_of(line, n):
    f = line.split(b"\t", 2)
    return int(f[0][1:].split(b"_")[0]) + (n if int(f[1]) & 0x80 else 0)


@pytest.mark.parametrize("k", [0, 1])
def test_pairs(k):
    c = cases.report_pair_case(*cases.REPORT_PAIR_CASES[k])
    cases.check_report_pair_case(c)
    dev = _device(c)
    try:
        dev.set_pairs(I, X)
        if c["E"] is not None:
            dev.set_rescue(c["E"])
        _stage(dev, c)
        off = _off(dev, c, paired=True)
        same_text(off["text"], cases.report_want(cases.REPORT_PAIR_CASES[k], True, False, False))
        for N in (1, m.ALL):
            on, n = _on(dev, off, N)
            with_xa = [l for l in on.splitlines() if m.xa_of(l)]
            assert any(m.flag_of(l) & 0x40 for l in with_xa) and any(m.flag_of(l) & 0x80 for l in with_xa)
            # a proper pair whose chosen record is not the mate's least-NM record: its entries hold a smaller NM than its own
            if N == m.ALL:
                assert any(m.flag_of(l) & 2 and min(int(e[4]) for e in m.entries(l)) < int(m.tag(l, b"NM:i")) for l in with_xa)
        off_slots = m.slots(off["text"])
        assert any(m.flag_of(s[0]) & 2 and len(s) > 1 and min(int(m.tag(l, b"NM:i")) for l in s[1:]) < int(m.tag(s[0], b"NM:i")) for s in off_slots)
        if c["E"] is not None:  # a rescued mate: one line and no XA
            rec_off = c["res"].rec_off
            rescued = [l for l in on.splitlines() if not m.flag_of(l) & 4 and rec_off[_read_of(l, c["n"]) + 1] == rec_off[_read_of(l, c["n"])]]
            assert rescued and dev.rescue_count() == len(rescued) and not any(m.xa_of(l) for l in rescued)
            assert all(l in off["text"].splitlines() for l in rescued)
    finally:
        dev.close()


# ---- 4. every option on ----

def test_every_option_on():
    c = dict(line_options_case(), e=LINE_E)
    dev = _device(c)
    try:
        pairing_on(dev, I, X, LINE_RESCUE_E)
        dev.set_report(strata=STRATA, max_hits=MAX_HITS)
        dev.set_tags(read_group=RG, hits=True)
        dev.set_mate_tags(True)
        dev.set_sam_seq(True)
        _stage(dev, c)
        off, on, n = _off_on(dev, c, m.ALL, paired=True)
        assert n > 0 and dev.filtered_count() > 0 and dev.rescue_count() > 0 and dev.unmapped_count() > 0
        with_xa = [l for l in on.splitlines() if m.xa_of(l)]
        assert with_xa and all(l.split(b"\t")[-2].startswith(b"ms:i:") for l in with_xa)  # the last field, behind ms:i
        placed = [l for l in off.splitlines() if m.flag_of(l) & 4 and l.split(b"\t")[2] != b"*"]
        assert placed and all(l in on.splitlines() for l in placed)
    finally:
        dev.close()


# ---- 5. * entries ----

def test_star_entries():
    c = m.star_case()
    assert m.star_secondaries(c)  # (the oracle: a slot with a secondary 0x8000 record)
    dev = _device(c)
    try:
        _stage(dev, c)
        off, on, n = _off_on(dev, c, m.ALL)
        starred =[e for l in on.splitlines() for e in m.entries(l) if e[3] == b"*"]
        assert len(starred) == len(m.star_secondaries(c))
        assert dev.fetch_sam()[2] >= len(starred)  # n_asserted counts the folded 0x8000 records
        assert {e[1] for e in starred} == {b"+", b"-"}
    finally:
        dev.close()


# ---- 6. staging and qualities ----

def test_packed_staging_and_host_qualities():
    c = m.equal_length_case()
    dev = _device(c)
    try:
        _stage(dev, c)
        off, on, n = _off_on(dev, c, m.ALL)
        assert n > 100
        _stage(dev, c, packed=True)
        off_p, on_p, n_p = _off_on(dev, c, m.ALL)
        assert (off_p, on_p, n_p) == (off, on, n)
        q, offsets = _stage(dev, c, quals_on_host=True)
        same_text(dev.fetch_sam(quals=q, offsets=offsets)[0], on)
        assert dev.xa_count() == n
        qa, nq = C.c_void_p(), C.c_uint64()
        dev._check(dev._L.fem_dev_sam_quals(dev._h, 0, C.byref(qa), C.byref(nq)))
        qual_at = np.ctypeslib.as_array(C.cast(qa.value, C.POINTER(C.c_uint64)), (nq.value,))
        at, seen, lines, starts = 0, 0, {}, {}
        for l in on.splitlines():  # (a read's first line is its primary one)
            lines.setdefault(l.split(b"\t", 1)[0], l)
            starts.setdefault(l.split(b"\t", 1)[0], at)
            at += len(l) + 1
        for r, (name, qual) in enumerate(zip(c["rnames"], c["quals"])):
            if name.encode() in lines:  # qual_at names the read's QUAL field, XA behind it or not
                l = lines[name.encode()]
                assert int(qual_at[r]) == starts[name.encode()] + len(b"\t".join(l.split(b"\t")[:10])) + 1
                seen += 1
            else:
                assert int(qual_at[r]) == 2 ** 64 - 1
        assert seen == len(lines) > 100
    finally:
        dev.close()


# ---- 7. stickiness and slots ----

def test_sticky_per_slot_off_again_and_the_refusal():
    c = cases.hits_case()
    dev = _device(c)
    try:
        _stage(dev, c, slot=0)
        _stage(dev, c, slot=1)
        off, on, n = _off_on(dev, c, m.ALL, slot=0)
        assert n > 0
        assert dev.fetch_sam(slot=1)[0] == off and dev.xa_count(slot=1) == 0  # the other slot's option is its own
        assert dev.fetch_sam(slot=0)[0] == on   # sticky
        _stage(dev, c, slot=0)
        assert dev.fetch_sam(slot=0)[0] == on and dev.xa_count(slot=0) == n  # ... over batches
        with pytest.raises(FemError):
            dev.set_xa(-1)
        assert dev.fetch_sam(slot=0)[0] == on   # (a refused call changes nothing)
        rec_on = dev.fetch_records(slot=0)
        dev.set_xa(0)
        assert dev.fetch_sam(slot=0)[0] == off and dev.xa_count(slot=0) == 0
        rec_off = dev.fetch_records(slot=0)
        for name in ("rec_begin", "flag", "tid", "pos0", "nm", "cigar_off", "cigar", "md_off", "md"):
            assert np.array_equal(getattr(rec_on, name), getattr(rec_off, name)), name
    finally:
        dev.close()


def test_kernel_time_id_18():
    c = cases.hits_case()
    dev = _device(c)
    try:
        dev.set_timing(True)
        _stage(dev, c)
        counts = lambda: [dev.kernel_time(k)[1] for k in range(3, 18)]  # noqa: E731  (0-2: the mapping, counted by the first fetch behind it)
        dev.reset_timing()
        dev.fetch_sam(), dev.fetch_bam(level=0)
        off_counts = counts()
        assert dev.kernel_time(18) == (0.0, 0)  # none with the option off
        dev.set_xa(m.ALL)
        dev.reset_timing()
        dev.fetch_sam(), dev.fetch_bam(level=0)
        ms, launches = dev.kernel_time(18)
        assert launches == 2 and ms > 0.0  # one entry per fetch: the text's and the BAM's
        assert counts() == off_counts      # ids 3-17 count as before (no filter is set: no 14, no 15)
        dev.set_report(max_hits=40)
        dev.reset_timing()
        dev.fetch_sam()
        assert dev.kernel_time(18)[1] == 1 and dev.kernel_time(15)[1] == 1
    finally:
        dev.close()


def test_fetch_pairs_is_unchanged():
    c = cases.report_pair_case(*cases.REPORT_PAIR_CASES[0])
    dev = _device(c)
    try:
        dev.set_pairs(I, X)
        _stage(dev, c)
        a = dev.fetch_pairs()
        dev.set_xa(2)
        b = dev.fetch_pairs()
        for name in ("rec_begin", "flag", "tid", "pos0", "nm", "cigar", "md", "mate_tid", "mate_pos0", "tlen", "stats"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert a.n_proper == b.n_proper
    finally:
        dev.close()


# ---- 8. a fixed slice of drawn option sets ----

def _set_options(dev, d, E):
    dev.set_pairs(I, X) if d["paired"] else dev.set_pairs(None)
    dev.set_rescue(E if d["paired"] and d["rescue"] else None)
    dev.set_rescue_discordant(bool(d["paired"] and d["rescue"] and d["discordant"]))
    dev.set_orientation(d["orientation"] if d["paired"] else 0)
    dev.set_mate_tags(bool(d["paired"] and d["mate_tags"]))
    dev.set_mapq(d["mapq"])
    dev.set_unmapped(d["unmapped"])
    dev.set_report(strata=d["strata"], max_hits=d["max_hits"])
    dev.set_tags(read_group=d["rg"], hits=d["hits"])
    dev.set_sam_seq(d["sam_seq"])


@pytest.mark.parametrize("k", range(len(m.DRAW_CASES)), ids=[x[0] for x in m.DRAW_CASES])
def test_drawn_option_sets(k):
    _, maker, args = m.DRAW_CASES[k]
    c = getattr(cases, maker)(*args)
    assert len(m.DRAW_CASES) * m.DRAWS_PER_CASE >= 16
    dev = _device(c)
    try:
        _stage(dev, c)
        texts, folded = set(), 0
        for d in m.draws(k):
            _set_options(dev, d, c.get("E") or 8)
            off, on, n = _off_on(dev, c, d["xa"], paired=d["paired"])
            texts.add(on)
            folded += n
        assert len(texts) >= 3 and folded > 0  # the draws differ in what they print
    finally:
        dev.close()


# ---- 9. FEM map --xa ----

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("xa")
    rng = np.random.default_rng(670)
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
    return dict(tmp=tmp, fa=str(fa), idx=idx_path, p1=str(p1), p2=str(p2), n=n)


def _n_gpus():
    import torch
    return torch.cuda.device_count()


@pytest.mark.parametrize("threads", [16, 24])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "read2"])
def test_cli(files, threads, paired):
    out = str(files["tmp"] / ("out_%d_%d" % (threads, paired)))
    common = ["-e", "2", "-t", str(threads), "--ref", files["fa"], "--index", files["idx"], "--read1", files["p1"], "--unmapped", "-o", out]
    if paired:
        common += ["--read2", files["p2"], "--rescue", "8", "--mate-tags"]

    def run(*args, bam=False):
        r = run_fem("map", *(common + list(args)))
        assert r.returncode == 0, r.stderr.decode()
        got = decode_bam_file(out) if bam else open(out, "rb").read()
        return b"".join(l + b"\n" for l in got.splitlines() if not l.startswith(b"@")), r.stderr

    def existing(stderr):
        return [l for l in counters(stderr) if not l.startswith("The number of XA entries")]

    plain, plain_err = run()
    assert not counter(plain_err, "XA entries")
    for args, N in ((("--xa",), m.ALL), (("--xa=2",), 2)):
        want, n = m.apply(plain, N)
        assert n > 200
        on, err = run(*args)
        same_text(on, want)
        assert existing(err) == existing(plain_err) == counters(plain_err) and counter(err, "XA entries") == [n]
        assert counters(err)[-1].startswith("The number of XA entries")  # behind the existing counter lines
    want, n = m.apply(plain, m.ALL)
    on_bam, err = run("--xa", "--bam", bam=True)
    same_text(on_bam, want)
    assert existing(err) == counters(plain_err) and counter(err, "XA entries") == [n]
    small, err = run("--xa", "--batch", "90")  # several batches: the same file, the count summed over them
    same_text(small, want)
    assert existing(err) == counters(plain_err) and counter(err, "XA entries") == [n]


def test_cli_two_gpus(files):
    if _n_gpus() < 2:
        pytest.skip("needs two devices")
    out = str(files["tmp"] / "out_g2")
    common = ["-e", "2", "-t", "16", "--ref", files["fa"], "--index", files["idx"], "--read1", files["p1"], "--batch", "90", "-o", out]
    r1 = run_fem("map", *(common + ["--xa"]))
    assert r1.returncode == 0, r1.stderr.decode()
    one = open(out, "rb").read()
    r2 = run_fem("map", *(common + ["--xa", "--gpus", "2"]))
    assert r2.returncode == 0, r2.stderr.decode()
    assert open(out, "rb").read() == one and counter(r2.stderr, "XA entries") == counter(r1.stderr, "XA entries")
