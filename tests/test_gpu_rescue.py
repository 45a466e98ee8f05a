"""Mate rescue on the device (fem_dev_set_rescue: the rescue kernels of fem_tail.hip in front of pair_kernel) against the
plain-Python model of tests/rescue_model.py on the oracle's single-end records.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import pair_model as pm
from tests import rescue_model as rm
from tests import util
from tests.cases import make_rescue_pairs, write_fastq
from tests.harness import build_index, counters, fetch_sam, open_device, open_reference, run_fem, same_pairs

pytestmark = pytest.mark.gpu


def _has_indel(rec):
    return any(op in "ID" for _, op in rec[4])


# seed, e, E, L, L2, n, repeats, X, quals on host, near sequence ends, packed staging
CASES = [
    (21, 2, 8, 100, 100, 600, False, 500, False, False, True),
    (22, 3, 15, 150, 150, 400, False, 500, True, True, True),
    (23, 2, 15, 250, 100, 300, True, 600, False, False, False),
    (24, 3, 3, 150, 150, 300, False, 500, False, False, False),
    (25, 2, 2, 100, 100, 300, True, 500, True, False, True),
    (26, 3, 8, 1000, 1000, 40, False, 3000, False, False, True),
    (27, 2, 8, 150, 100, 400, True, 500, True, False, False),
]


@pytest.mark.parametrize("seed,e,E,L,L2,n,repeats,X,qhost,near_end,packed", CASES)
def test_rescued_text_equals_the_model(seed, e, E, L, L2, n, repeats, X, qhost, near_end, packed):
    rng, dev, ref, idx, seqs, names = open_reference(seed, repeats)
    try:
        r1, r2 = make_rescue_pairs(rng, seqs, n, L, L2, e, E, X, near_end=near_end)
        reads = r1 + r2
        rnames = ["p%d" % i for i in range(n)] * 2
        quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
        want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
        I = 0
        ext, kept, _ = rm.rescue(want, n, reads, seqs, E, I, X)
        if E > e:  # the fixture really rescues: both orientations, both mates as the anchor, an indel through the walk
            assert sum(k["rc"] for k in kept.values()) > 0 and sum(not k["rc"] for k in kept.values()) > 0
            assert any(r < n for r in kept) and any(r >= n for r in kept)
            assert any(_has_indel(k["record"]) for k in kept.values())
            if repeats:  # several anchors
                cnt = np.diff(want.rec_off.astype(np.int64))
                assert any(cnt[r - n if r >= n else r + n] > 1 for r in kept)
        dev.set_pairs(I, X, slot=1)
        dev.set_rescue(E, slot=1)
        dev.set_timing(True)
        dev.reset_timing()
        text, n_records, _, stats = fetch_sam(dev, reads, rnames, quals, e, 1, qhost, packed)
        assert np.array_equal(stats, want.stats) and n_records == int(want.rec_off[-1])  # single-end meaning kept
        exp = pm.sam_lines(ext, n, names, reads, rnames, quals, I, X)
        assert text.decode("latin-1") == exp
        _, n_proper = pm.expected(ext, n, I, X)
        assert dev.pair_count(slot=1) == n_proper and dev.rescue_count(slot=1) == len(kept)
        assert dev.kernel_time(10)[1] >= 1
        same_pairs(dev.fetch_pairs(slot=1), pm.pair_arrays(ext, n, I, X))
        assert dev.rescue_count(slot=1) == len(kept)
        rec = dev.fetch_records(slot=1)  # single-end records untouched
        assert rec.n_records == int(want.rec_off[-1])
        if seed == 21:
            # rescue off again: byte-identical to a slot that never had it
            dev.set_rescue(None, slot=1)
            text_off, _, _, _ = fetch_sam(dev, reads, rnames, quals, e, 1, qhost, packed)
            dev.set_pairs(I, X, slot=0)
            text_0, _, _, _ = fetch_sam(dev, reads, rnames, quals, e, 0, qhost, packed)
            assert text_off == text_0 and text_off.decode("latin-1") == pm.sam_lines(want, n, names, reads, rnames, quals, I, X)
            assert dev.rescue_count(slot=1) == 0
            # rescue on, no candidate pair (both mates mapped everywhere): unchanged text
            cnt = np.diff(want.rec_off.astype(np.int64))
            both = [i for i in range(n) if cnt[i] > 0 and cnt[n + i] > 0]
            sub = [reads[i] for i in both] + [reads[n + i] for i in both]
            sq = [quals[i] for i in both] + [quals[n + i] for i in both]
            sn = ["p%d" % i for i in both] * 2
            dev.set_rescue(E, slot=1)
            t_on, _, _, _ = fetch_sam(dev, sub, sn, sq, e, 1)
            t_off, _, _, _ = fetch_sam(dev, sub, sn, sq, e, 0)
            assert t_on == t_off and dev.rescue_count(slot=1) == 0
    finally:
        dev.close()


@pytest.mark.parametrize("seed,E,L", [(41, 8, 150), (42, 15, 250)])
def test_soft_masked_reference_and_lower_case_reads(seed, E, L):
    """Lower-case characters on either side: the search compares codes, the traceback and MD characters, so a rescued mate's
    MD can hold every column — more than the first traceback pass stages; the overflow pass takes those records."""
    rng = np.random.default_rng(seed)
    s0 = util.rand_seq(rng, 200_000)
    seqs = [s0[:20_000] + s0[20_000:140_000].lower() + s0[140_000:], util.rand_seq(rng, 60_000)]
    names = ["chr0", "chr1"]
    dev, ref, idx = open_device(seqs, names)
    try:
        e, n, X = 2, 400, 600
        r1, r2 = make_rescue_pairs(rng, seqs, n, L, L, e, E, X)
        reads = [r.lower() if i % 3 == 0 else r.upper() for i, r in enumerate(r1 + r2)]
        rnames = ["s%d" % i for i in range(n)] * 2
        quals = ["".join(chr(35 + (7 * i + j) % 50) for j in range(len(r))) for i, r in enumerate(reads)]
        want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
        ext, kept, _ = rm.rescue(want, n, reads, seqs, E, 0, X)
        long_md = [k for k in kept.values() if len(k["record"][5]) > 8 * E + 64]
        assert len(long_md) >= 2 and len(kept) > len(long_md)  # both traceback passes
        dev.set_pairs(0, X)
        dev.set_rescue(E)
        text, _, _, _ = fetch_sam(dev, reads, rnames, quals, e, 0)
        assert text.decode("latin-1") == pm.sam_lines(ext, n, names, reads, rnames, quals, 0, X)
        _, n_proper = pm.expected(ext, n, 0, X)
        assert dev.pair_count() == n_proper and dev.rescue_count() == len(kept)
        same_pairs(dev.fetch_pairs(), pm.pair_arrays(ext, n, 0, X))
    finally:
        dev.close()


def test_refusals():
    from fem_amd import FemError
    rng, dev, ref, idx, seqs, names = open_reference(28, False)
    try:
        for bad in (-1, 16):
            with pytest.raises(FemError):
                dev.set_rescue(bad)
        r1, r2 = make_rescue_pairs(rng, seqs, 20, 100, 100, 2, 8, 500)
        reads = r1 + r2
        quals = ["I" * len(r) for r in reads]
        rnames = ["o%d" % i for i in range(20)] * 2
        dev.set_pairs(100, 100 + 65537)
        dev.set_rescue(8)
        with pytest.raises(FemError):
            fetch_sam(dev, reads, rnames, quals, 2, 0, packed=True)
        dev.set_pairs(100, 100 + 65536)  # the widest window rescue searches
        text, _, _, _ = fetch_sam(dev, reads, rnames, quals, 2, 0, packed=True)
        want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=2)
        ext, kept, _ = rm.rescue(want, 20, reads, seqs, 8, 100, 100 + 65536)
        assert text.decode("latin-1") == pm.sam_lines(ext, 20, names, reads, rnames, quals, 100, 100 + 65536)
    finally:
        dev.close()


# ---- FEM map --rescue ----

def _map(fa, idx_path, p1, p2, out, *extra):
    return run_fem("map", "-e", "2", "-t", "4", "--ref", fa, "--index", idx_path, "--read1", p1, "--read2", p2, "-o", out, *extra,
                   text=True)


@pytest.mark.parametrize("gz", [False, True])
def test_cli_rescue_equals_the_model(tmp_path, gz):
    rng = np.random.default_rng(31 + gz)
    seqs = [util.rand_seq(rng, 150_000), util.rand_seq(rng, 60_000)]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = tmp_path / "ref.idx"
    build_index(fa, idx_path)
    n = 2000
    r1, r2 = make_rescue_pairs(rng, seqs, n, 100, 100, 2, 8, 500, frac=0.1)
    base = ["pair%d" % i for i in range(n)]
    q1 = ["".join(chr(33 + (7 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r1)]
    q2 = ["".join(chr(34 + (5 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(r2)]
    ext_ = ".fq.gz" if gz else ".fq"
    p1, p2 = tmp_path / ("r1" + ext_), tmp_path / ("r2" + ext_)
    write_fastq(p1, r1, [b + "/1" for b in base], q1, gz)
    write_fastq(p2, r2, [b + "/2" for b in base], q2, gz)
    ref = fo.Reference(seqs)
    want = fo.map_reads(ref, fo.OracleIndex(ref), fo.ReadBatch(r1 + r2), e=2, threads=4)
    ext, kept, _ = rm.rescue(want, n, r1 + r2, seqs, 8, 0, 500)
    assert len(kept) > 50
    header = "".join("@SQ\tSN:s%d\tLN:%d\n" % (i, len(s)) for i, s in enumerate(seqs))
    out = tmp_path / "out.sam"
    r = _map(fa, idx_path, p1, p2, out, "--batch", "700", "--rescue", "8")
    assert r.returncode == 0, r.stderr
    assert out.read_text(encoding="latin-1") == header + pm.sam_lines(ext, n, ["s0", "s1"], r1 + r2, base + base, q1 + q2, 0, 500)
    _, n_proper = pm.expected(ext, n, 0, 500)
    assert counters(r.stderr)[-2:] == ["The number of proper pairs: %d" % n_proper, "The number of rescued mates: %d" % len(kept)]
    # without the flag: the output of a paired run, no rescue line
    out0 = tmp_path / "out0.sam"
    r = _map(fa, idx_path, p1, p2, out0, "--batch", "700")
    assert r.returncode == 0, r.stderr
    assert out0.read_text(encoding="latin-1") == header + pm.sam_lines(want, n, ["s0", "s1"], r1 + r2, base + base, q1 + q2, 0, 500)
    assert "rescued" not in r.stderr


def test_fetch_timing_counts():
    """With timing on, every fetch advances the launch counts of exactly its kernel-time ids (include/fem_hip.h), by one
    each: fetch_records 3-5; fetch_sam 3-5 and 7 when it waits; fetch_bam 3-5, 11 and 12; a text of read pairs also 9, and
    10 with mate rescue."""
    rng, dev, ref, idx, seqs, names = open_reference(28, False)
    try:
        n, e = 150, 2
        r1, r2 = make_rescue_pairs(rng, seqs, n, 100, 100, e, 8, 500)
        reads = r1 + r2
        batch = fo.ReadBatch(reads)
        q = np.full(len(batch.bases), ord("I"), np.uint8)
        dev.set_pairs(0, 500, slot=1)
        dev.set_rescue(8, slot=1)
        dev.set_pairs(0, 500, slot=2)
        dev.set_timing(True)

        def advanced(fetch):
            before = [dev.kernel_time(k)[1] for k in range(16)]
            fetch()
            after = [dev.kernel_time(k)[1] for k in range(16)]
            return {k: after[k] - before[k] for k in range(16) if after[k] != before[k]}

        for slot, paired, rescue in ((0, False, False), (1, True, True), (2, True, False)):
            dev.stage_reads(batch.bases, batch.off, slot=slot)
            dev.stage_text(q, ["r%d" % i for i in range(2 * n)], slot=slot)
            dev.map_staged(e=e, slot=slot)
            dev.sync(slot)
            text_ids = {3, 4, 5} | ({9} if paired else set()) | ({10} if rescue else set())
            assert advanced(lambda: dev.fetch_records(slot=slot)) == dict.fromkeys({3, 4, 5}, 1)
            assert advanced(lambda: dev.fetch_sam(slot=slot)) == dict.fromkeys(text_ids | {7}, 1)
            assert advanced(lambda: dev.fetch_sam(slot=slot, nowait=True)) == dict.fromkeys(text_ids, 1)
            assert advanced(lambda: dev.fetch_bam(slot=slot)) == dict.fromkeys(text_ids | {11, 12}, 1)
    finally:
        dev.close()


def test_fetch_timing_counts_with_every_stage():
    """A paired slot with rescue, MAPQ and lines for unmapped reads, over all sixteen ids: with the line filter a waiting
    fetch_sam counts 3-5, 7, 9, 10, 13 and 15 (the filter's line index is the unmapped reads' too: no 14); without the
    filter a fetch_bam that does not wait counts 3-5, 9-14."""
    rng, dev, ref, idx, seqs, names = open_reference(28, False)
    try:
        n, e = 150, 2
        r1, r2 = make_rescue_pairs(rng, seqs, n, 100, 100, e, 8, 500)
        batch = fo.ReadBatch(r1 + r2)
        q = np.full(len(batch.bases), ord("I"), np.uint8)
        dev.set_pairs(0, 500, slot=1)
        dev.set_rescue(8, slot=1)
        dev.set_mapq(True, slot=1)
        dev.set_unmapped(True, slot=1)
        dev.set_timing(True)
        dev.stage_reads(batch.bases, batch.off, slot=1)
        dev.stage_text(q, ["r%d" % i for i in range(2 * n)], slot=1)
        dev.map_staged(e=e, slot=1)
        dev.sync(1)

        def advanced(fetch):
            before = [dev.kernel_time(k)[1] for k in range(16)]
            fetch()
            after = [dev.kernel_time(k)[1] for k in range(16)]
            return {k: after[k] - before[k] for k in range(16) if after[k] != before[k]}

        dev.set_report(strata=0, slot=1)
        assert advanced(lambda: dev.fetch_sam(slot=1)) == dict.fromkeys({3, 4, 5, 7, 9, 10, 13, 15}, 1)
        dev.set_report(slot=1)
        assert advanced(lambda: dev.fetch_bam(slot=1, nowait=True)) == dict.fromkeys({3, 4, 5, 9, 10, 11, 12, 13, 14}, 1)
    finally:
        dev.close()
