"""RG:Z, NH:i and HI:i on the device (fem_dev_set_tags: the tag parts of the text and BAM record kernels, fem_tail.hip) and the
header of FEM map --header / --rg against the plain-Python rule of tests/tags_model.py, applied to what the other models expect
of the same batch without tags.  Needs a GPU: -m gpu."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import bam_model as bm
from tests import report_model as rp
from tests import tags_model as tm
from tests import unmapped_model as um
from tests import util
from tests.cases import I, X, hits_case, make_pairs, quals, report_want, write_fastq
from tests.cases import REPORT_PAIR_CASES as PAIR_CASES, REPORT_SINGLE_CASES as SINGLE_CASES
from tests.cases import report_pair_case as pair_case, report_single_case as single_case
from tests.harness import FEM, ROOT, build_index, decode_bam_file, fetch_sam, open_device, run_fem, same_text, set_line_filter
from tests.harness import stage_and_map

pytestmark = pytest.mark.gpu

# ID lengths: one byte, a wave's width and the bytes around it, the longest
IDS = {k: bytes(33 + (7 * i + k) % 94 for i in range(k)) for k in (1, 63, 64, 65, 255)}
IDS[6] = b"lane 1"


# ---- the device's text and BAM against the model ----

def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _stage(dev, c, slot, quals_on_host=False):
    return stage_and_map(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, quals_on_host)


def _sam(dev, c, slot, quals_on_host=False):
    return fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, quals_on_host)


def _bam(dev, slot, ref_names, text):
    """fetch_bam of the slot's staged batch at both levels: the model's records of `text`, which decode to it."""
    want = tm.bam_payload(text, ref_names)
    for level in (0, 1):
        data = dev.fetch_bam(slot=slot, level=level)
        payload = b"".join(m[0] for m in bm.parse_bgzf(data[0], eof=False)) if data[0] else b""
        assert data[1] == len(want)
        assert payload == want
    assert bm.bam_payload_to_sam(want, ref_names) == text


def _check(dev, c, slot, model, rg, hits, quals_on_host=False):
    """The slot's text and BAM with these tags == the model's tags on `model` (the expected text without them) -> the text."""
    dev.set_tags(slot=slot, read_group=rg, hits=hits)
    want = tm.apply(model, rg, hits)
    got = _sam(dev, c, slot)[0]
    same_text(got, want)
    _bam(dev, slot, [x.encode() for x in c["names"]], want)
    if quals_on_host:  # qual_at still finds every QUAL field: the tags stand behind it
        same_text(_sam(dev, c, slot, quals_on_host=True)[0], want)
    return got


# ---- wave boundaries of the write kernels and ID lengths: batches of exactly n lines ----

UNIQUE_SEQ = util.rand_seq(np.random.default_rng(300), 30_000)


@functools.lru_cache(maxsize=None)
def unique_case(n, lost=False):
    """n reads that map exactly once each (lost: every third one of random letters instead, which maps nowhere)."""
    rng = np.random.default_rng(301 + n)
    starts = rng.choice(np.arange(220, len(UNIQUE_SEQ) - 330, 110), n, replace=False)
    reads = [UNIQUE_SEQ[s:s + 100] if i % 2 else util.revcomp(UNIQUE_SEQ[s:s + 100]) for i, s in enumerate(starts)]
    if lost:
        reads = [util.rand_seq(rng, 100) if i % 3 == 1 else r for i, r in enumerate(reads)]
    rnames = ["u%d_%s" % (i, "n" * (i % 7)) for i in range(n)]
    ref = fo.Reference([UNIQUE_SEQ])
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=3, threads=4)
    counts = np.diff(res.rec_off.astype(np.int64))
    assert all(int(k) == (0 if lost and i % 3 == 1 else 1) for i, k in enumerate(counts)), counts
    return dict(seqs=[UNIQUE_SEQ], names=["uniq"], reads=reads, rnames=rnames, quals=quals(reads), e=3, idx=idx, res=res)


@pytest.fixture(scope="module")
def unique_dev():
    dev = _device(unique_case(1))
    yield dev
    dev.close()


@pytest.mark.parametrize("n,k", [(1, 255), (2, 65), (63, 64), (64, 63), (65, 1), (129, 255)])
def test_wave_boundaries(unique_dev, n, k):
    dev = unique_dev
    for lost in (False, True):
        c = unique_case(n, lost)
        set_line_filter(dev, 0, False, lost, None, None)
        model = um.single_end(c["res"], c["names"], c["reads"], c["rnames"], c["quals"])
        if not lost:
            model = um.without_unmapped(model)[0]
        assert model.count(b"\n") == n
        got = _check(dev, c, 0, model, IDS[k], True, quals_on_host=True)
        assert got.count(b"\n") == n and got.count(b"\tRG:Z:" + IDS[k] + b"\n") == n
        assert got.count(b"\tNH:i:1\tHI:i:1\t") == n - ((n + 1) // 3 if lost else 0)


@pytest.mark.parametrize("k", sorted(IDS))
def test_id_lengths(unique_dev, k):
    dev, c = unique_dev, unique_case(65)
    set_line_filter(dev, 0, False, False, None, None)
    model = um.without_unmapped(um.single_end(c["res"], c["names"], c["reads"], c["rnames"], c["quals"]))[0]
    for hits in (False, True):
        _check(dev, c, 0, model, IDS[k], hits)


# ---- hit counts: slots of 130 lines among slots of 1 and 2 ----

@pytest.mark.parametrize("strata,max_hits", [(None, None), (0, None), (None, 1), (None, 33), (None, 100)])
def test_hit_counts(strata, max_hits):
    c = hits_case()
    base = um.without_unmapped(um.single_end(c["res"], c["names"], c["reads"], c["rnames"], c["quals"]))[0]
    model = rp.apply(base, strata, max_hits)[0]
    kept = 130 if max_hits is None else min(130, max_hits)  # NH is what is in the text, not what was found
    dev = _device(c)
    try:
        set_line_filter(dev, 0, False, False, strata, max_hits)
        got = _check(dev, c, 0, model, IDS[6], True)
        for hi in sorted({1, 9, 10, 32, 33, 64, 65, 99, 100, 130, kept}):
            assert got.count(b"\tNH:i:%d\tHI:i:%d\t" % (kept, hi)) == ((16 if kept == 1 else 5) if hi <= kept else 0), hi
        assert (b"\tNH:i:130\t" in got) == (kept == 130)
        assert got.count(b"\tNH:i:2\tHI:i:2\t") == (4 if kept >= 2 else 0) and got.count(b"\tNH:i:1\tHI:i:1\t") == (16 if kept == 1 else 7)
        _check(dev, c, 0, model, None, True)
    finally:
        dev.close()


# ---- every line shape: the --strata / --max-hits cases of tests/cases.py, a sampled matrix of the switches ----

# case, paired, mapq, unmapped, ID length (None: no RG), NH / HI, (S, N) of the line filter
MATRIX = [
    (SINGLE_CASES[0], False, False, False, 6, True, (None, None)),
    (SINGLE_CASES[0], False, True, True, 65, True, (None, None)),
    (SINGLE_CASES[0], False, False, True, None, True, (1, 3)),
    (SINGLE_CASES[0], False, True, False, 255, False, (None, 33)),
    (PAIR_CASES[0], True, False, True, 6, True, (None, None)),
    (PAIR_CASES[0], True, True, False, None, True, (None, None)),
    (PAIR_CASES[0], True, True, True, 64, False, (0, None)),
    (PAIR_CASES[1], True, True, True, 6, True, (None, None)),
    (PAIR_CASES[1], True, False, False, 63, True, (None, None)),
    (PAIR_CASES[1], True, False, True, 1, True, (None, 2)),
    (PAIR_CASES[1], True, True, True, None, True, (2, 64)),
    (PAIR_CASES[1], True, False, False, 6, False, (None, None)),
]


def _shapes(text, paired):
    """Which shapes of line `text` holds."""
    found = set()
    for l in text.split(b"\n")[:-1]:
        f = l.split(b"\t")
        flag = int(f[1])
        if flag & 4:
            found.add("unplaced" if f[2] == b"*" else "placed")
        else:
            found.add("secondary" if flag & 256 else "primary")
            if paired and flag & 8 and f[6] != b"*":
                found.add("mate of a placed one")
            if f[5] == b"*":
                found.add("0x8000")
    return found


@pytest.mark.parametrize("row", range(len(MATRIX)), ids=lambda i: "row%d" % i)
def test_every_line_shape(row):
    case, paired, mapq, unmapped, k, hits, flt = MATRIX[row]
    c = pair_case(*case) if paired else single_case(*case)
    model = rp.apply(report_want(case, paired, mapq, unmapped), *flt)[0]
    shapes = _shapes(model, paired)
    assert {"primary", "secondary"} <= shapes
    if unmapped:
        assert "unplaced" in shapes and (not paired or {"placed", "mate of a placed one"} <= shapes)
    dev = _device(c)
    try:
        if paired:
            dev.set_pairs(I, X, slot=1)
            if c["E"] is not None:
                dev.set_rescue(c["E"], slot=1)
        set_line_filter(dev, 1, mapq, unmapped, *flt)
        got = _check(dev, c, 1, model, None if k is None else IDS[k], hits, quals_on_host=hits and k is not None)
        if paired and c["E"] is not None and hits:  # a rescued mate's record is its slot's only line
            assert dev.rescue_count(slot=1) == len(c["kept"]) >= 20
            assert got.count(b"\tNH:i:1\tHI:i:1") >= len(c["kept"])
    finally:
        dev.close()


# ---- records the reference would have asserted on (0x8000: CIGAR *, MD empty): lines like any other, counted by NH ----

@pytest.mark.parametrize("paired", [False, True], ids=["single", "pairs"])
def test_asserted_records(paired):
    c = tm.asserted_case()
    n = len(c["reads"])
    with_unm = um.paired(c["res"], n // 2, c["names"], c["reads"], c["rnames"], c["quals"], I, X) if paired else \
        um.single_end(c["res"], c["names"], c["reads"], c["rnames"], c["quals"])
    n_asserted = int(np.count_nonzero(c["res"].r_flag & 0x8000))
    assert n_asserted >= 10
    dev = _device(c)
    try:
        if paired:
            dev.set_pairs(I, X, slot=1)
        for unmapped in (False, True):
            plain = with_unm if unmapped else um.without_unmapped(with_unm, paired)[0]
            assert {"primary", "secondary", "0x8000"} <= _shapes(plain, paired)
            assert sum(1 for l in plain.split(b"\n")[:-1] if l.split(b"\t")[5] == b"*" and not int(l.split(b"\t")[1]) & 4) == n_asserted
            for flt in ((None, None), (0, None), (None, 2)):
                model = rp.apply(plain, *flt)[0]
                set_line_filter(dev, 1, False, unmapped, *flt)
                got = _check(dev, c, 1, model, IDS[6], True, quals_on_host=True)
                _check(dev, c, 1, model, None, True)
                # the 0x8000 lines: MD:Z: empty, then NH and HI; a slot's count includes them, and they have a place of their own
                marked = [l for l in got.split(b"\n")[:-1] if b"\tMD:Z:\tNH:i:" in l]
                assert len(marked) == sum(1 for l in model.split(b"\n")[:-1] if l.endswith(b"\tMD:Z:")) >= 3
                if flt == (None, None):
                    assert len(marked) == n_asserted
                    his = [int(re.search(rb"\tHI:i:(\d+)", l).group(1)) for l in marked]
                    nhs = [int(re.search(rb"\tNH:i:(\d+)", l).group(1)) for l in marked]
                    assert any(h > 1 for h in his) and any(h == 1 for h in his) and max(nhs) >= 3
                    assert all(1 <= h <= k for h, k in zip(his, nhs))
    finally:
        dev.close()


# ---- nothing maps, an empty batch ----

def test_nothing_maps_and_an_empty_batch():
    rng = np.random.default_rng(320)
    c = dict(seqs=[util.rand_seq(rng, 5000)], names=["tiny"], e=3)
    c["reads"] = [util.rand_seq(rng, int(rng.integers(30, 160))) for _ in range(200)]
    c["rnames"] = ["x%d" % i for i in range(200)]
    c["quals"] = quals(c["reads"])
    ref = fo.Reference(c["seqs"])
    c["idx"] = fo.OracleIndex(ref)
    res = fo.map_reads(ref, c["idx"], fo.ReadBatch(c["reads"]), e=3, threads=4)
    assert int(res.rec_off[-1]) == 0
    empty = dict(c, reads=[], rnames=[], quals=[])
    dev = _device(c)
    try:
        dev.set_tags(read_group=IDS[65], hits=True)
        assert _sam(dev, c, 0)[0] == b""
        _bam(dev, 0, [b"tiny"], b"")
        dev.set_unmapped(True)
        model = um.single_end(res, c["names"], c["reads"], c["rnames"], c["quals"])
        got = _check(dev, c, 0, model, IDS[65], True, quals_on_host=True)
        assert got.count(b"\n") == 200 == got.count(b"\tRG:Z:" + IDS[65] + b"\n") and b"NH:i" not in got and b"HI:i" not in got
        dev.set_pairs(I, X)
        _check(dev, c, 0, um.paired(res, 100, c["names"], c["reads"], c["rnames"], c["quals"]), IDS[65], True)
        for pairs in (False, True):
            dev.set_pairs(I, X) if pairs else dev.set_pairs(None)
            for unmapped in (False, True):
                dev.set_unmapped(unmapped)
                for flt in ((None, None), (0, 1)):
                    dev.set_report(*flt)
                    assert _sam(dev, empty, 0)[0] == b""
                    _bam(dev, 0, [b"tiny"], b"")
    finally:
        dev.close()


# ---- off again, invalid parameters ----

def test_off_again_and_invalid_parameters():
    from fem_amd import FemError
    c = unique_case(129, True)
    dev = _device(c)
    try:
        dev.set_unmapped(True, slot=0)
        dev.set_unmapped(True, slot=1)
        off = _sam(dev, c, 0)[0]
        bam_off = [dev.fetch_bam(slot=0, level=level)[0] for level in (0, 1)]
        assert tm.strip(off) == (off, [(None, None, None)] * 129)
        on = _check(dev, c, 1, off, IDS[6], True)
        assert on != off
        dev.set_tags(slot=1)  # NULL: off, byte for byte the text and the BAM of a slot that never had tags
        assert _sam(dev, c, 1)[0] == off
        assert [dev.fetch_bam(slot=1, level=level)[0] for level in (0, 1)] == bam_off
        _check(dev, c, 1, off, IDS[1], False)
        from fem_amd.device import _TagParams
        for bad in (b"", b"i" * 256, b"a\tb", b"caf\xe9", b"\x7f", b"new\nline"):
            with pytest.raises(FemError, match=r"^invalid argument: read group ID"):  # (fem_strerror(FEM_ERR_INVALID): the reason)
                dev.set_tags(slot=1, read_group=bad, hits=True)
            tp = _TagParams(bad, 1)
            assert dev._L.fem_dev_set_tags(dev._h, 1, ctypes.byref(tp)) == -1  # FEM_ERR_INVALID
        assert _sam(dev, c, 1)[0] == tm.apply(off, IDS[1], False)  # (a refused call leaves the slot's setting as it was)
        # the ID was copied at the call
        rg = bytearray(b"first")
        dev.set_tags(slot=1, read_group=bytes(rg), hits=False)
        rg[:] = b"other"
        assert _sam(dev, c, 1)[0] == tm.apply(off, b"first", False)
        # the records are what they are without tags
        dev.set_tags(slot=1, read_group=IDS[6], hits=True)
        _stage(dev, c, 1)
        assert dev.fetch_records(slot=1).n_records == int(c["res"].rec_off[-1])
    finally:
        dev.close()


# ---- FEM map --header / --rg / --nh ----

def _version():
    return re.search(r'#define FEM_VERSION "([^"]+)"', open(os.path.join(ROOT, "fem_amd", "csrc", "fem_main.cc")).read()).group(1)


def _split_header(data):
    lines = data.split(b"\n")
    k = next((i for i, l in enumerate(lines) if not l.startswith(b"@")), len(lines))
    return b"".join(l + b"\n" for l in lines[:k]), b"\n".join(lines[k:])


def test_cli(tmp_path):
    rng = np.random.default_rng(331)
    seqs = util.repeat_rich_reference(rng, n_seq=2, unit_len=300, n_units=3, copies=12, spacer=200) + [util.rand_seq(rng, 60_000)]
    names = ["s%d" % i for i in range(len(seqs))]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = str(tmp_path / "ref.idx")
    build_index(fa, idx_path)
    sq = "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, len(s)) for nm, s in zip(names, seqs)).encode()
    n, e = 400, 3
    se = util.make_reads(rng, seqs, n, 100, e)
    x1, x2 = make_pairs(rng, seqs, n, 100, e)
    for i in range(n):
        u = rng.random()
        if u < 0.2:
            se[i] = util.rand_seq(rng, 100)
        if u < 0.15:
            x1[i] = util.rand_seq(rng, 100)
        if u < 0.05 or u > 0.95:
            x2[i] = util.rand_seq(rng, 100)
    q = ["".join(chr(33 + (7 * i + j) % 40) for j in range(100)) for i in range(n)]
    rn = ["r%d" % i for i in range(n)]
    files = {}
    for key, reads, suffix in (("se", se, ""), ("x1", x1, "/1"), ("x2", x2, "/2")):
        files[key] = tmp_path / (key + ".fq")
        write_fastq(files[key], reads, [x + suffix for x in rn], q, False)
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(se), e=e, threads=8)
    want_se = rp.single_end(res, names, se, rn, q, unmapped=False)[0]
    resp = fo.map_reads(ref, idx, fo.ReadBatch(x1 + x2), e=e, threads=8)
    want_pe = rp.paired(resp, n, names, x1 + x2, rn + rn, q + q, I, X, max_hits=2)[0]
    assert _shapes(want_pe, True) >= {"primary", "secondary", "unplaced", "placed", "mate of a placed one"}
    common = ["-e", str(e), "-t", "4", "--ref", str(fa), "--index", idx_path, "--batch", "150"]
    single = ["--read1", str(files["se"])]
    pairs = ["--read1", str(files["x1"]), "--read2", str(files["x2"]), "--unmapped", "--max-hits", "2"]
    out = str(tmp_path / "out")
    runs = [  # arguments, BAM, the --rg argument, NH / HI, the text without tags, @HD and @PG
        (single + ["--rg", "@RG\\tID:lane.1\\tSM:sample one", "--nh"], False, "@RG\\tID:lane.1\\tSM:sample one", True, want_se, True),
        (pairs + ["--bam", "--rg", "@RG\tID:L2\tPL:x", "--nh", "--gpus", "2"], True, "@RG\tID:L2\tPL:x", True, want_pe, True),
        (single + ["--header"], False, None, False, want_se, True),
        (single, False, None, False, want_se, False),  # without the switches: no @HD, no @PG, no tags
    ]
    for args, bam, rg_arg, hits, plain, hd in runs:
        args = common + args + ["-o", out]
        r = run_fem("map", *args, env={"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"})  # (--gpus 2: two workers on the one GPU)
        assert r.returncode == 0, r.stderr.decode()
        got = decode_bam_file(out) if bam else open(out, "rb").read()
        header, body = _split_header(got)
        rg = None if rg_arg is None else re.search(r"ID:([^\t]+)", tm.rg_line(rg_arg).decode()).group(1).encode()
        if hd:
            assert header == tm.header(sq, None if rg_arg is None else tm.rg_line(rg_arg), tm.pg_line([FEM, "map"] + args, _version()))
        else:
            assert header == sq
        # (the batches' texts arrive in any order; a batch is whole reads / whole pairs, so every slot's lines stay together)
        want = tm.apply(plain, rg, hits)
        assert sorted(body.splitlines()) == sorted(want.splitlines())
        stripped, tags = tm.strip(body)
        assert tm.apply(stripped, rg, hits) == body
        if rg is None and not hits:
            assert stripped == body
