"""Size-independent properties of the device path at BASELINE.json's sizes (no oracle needed at this scale),
plus a statistical cross-check against the SURVEY's probe of the true reference binary.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from fem_amd import host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from fem_amd import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def c2(dev):
    # BASELINE.json configs[1] shape: 5 Mbp reference, 100 bp reads, e=3 (2 M reads here; bench.py runs the 10 M)
    text, off, lens = host.synth_reference(2, [5_000_000], threads=16)
    dev.upload_reference([text[:5_000_000]])
    dev.build_index(12, 3, fetch=False)
    n = 2_000_000
    bases, offs = host.synth_reads(2, text, off, lens, n, 100, 3, threads=16)
    return text, off, lens, bases, offs, n


def test_counters_are_consistent_with_the_result_arrays(dev, c2):
    text, off, lens, bases, offs, n = c2
    r = dev.map_batch(bases, offs, e=3)
    o, cand, ed, end = r.per_strand()
    assert int(r.stats[0]) == n
    assert int(r.stats[3]) == len(cand) == int(r.cand_count.sum())
    assert int(r.stats[4]) == int(np.count_nonzero(ed != 0xFF))
    acc = np.add.reduceat(np.concatenate([(ed != 0xFF).astype(np.int64), [0]]), o[:-1].astype(np.int64))
    acc[np.diff(o.astype(np.int64)) == 0] = 0
    per_read = acc[0::2] + acc[1::2]
    assert int(r.stats[1]) == int(np.count_nonzero(per_read))
    assert np.all(ed[ed != 0xFF] <= 3)
    assert np.all((end[ed != 0xFF] >= 99) & (end[ed != 0xFF] <= 99 + 6))  # end offset in [L-1, L-1+2e]
    # candidates of a strand are strictly ascending and more than e apart (staged greedy, src/filter.c:45-78)
    d = np.diff(cand.astype(np.int64))
    inner = np.ones(len(cand) - 1, bool)
    inner[(o[1:-1] - 1).astype(np.int64)[(o[1:-1] > 0) & (o[1:-1] < len(cand))]] = False
    assert np.all(d[inner] > 3)
    assert int(r.stats[1]) > 0.8 * n  # reads come from the reference with <= e edits: most of them map


def test_c2_workload_array_for_array_against_the_oracle(dev, c2):
    # the first 200 k reads of the C2 workload (the bench's generator, seed 2): candidates, edit distances, end offsets
    # and counters of the device path — seed_fast_kernel<lean>, as the library selects it — equal the oracle's
    from oracle import fem_oracle as fo
    text, off, lens, bases, offs, n = c2
    m = 200_000
    assert dev.seed_kernel(e=3) == "seed_fast_kernel<lean>"
    ref = fo.Reference([text[:5_000_000].tobytes()])
    idx = fo.OracleIndex(ref)
    sub_b, sub_o = bases[:int(offs[m]) + 8], offs[:m + 1]
    want = fo.map_reads(ref, idx, fo.ReadBatch.from_arrays(sub_b, sub_o), e=3, a=1, threads=16, stages=fo.STAGE_SEED | fo.STAGE_VERIFY)
    got = dev.map_batch(sub_b, sub_o, e=3, slot=2)
    o, cand, ed, end = got.per_strand()
    assert np.array_equal(got.stats, want.stats), (got.stats, want.stats)
    assert np.array_equal(o, want.cand_off) and np.array_equal(cand, want.cands)
    assert np.array_equal(ed, want.v_ed) and np.array_equal(end[ed != 0xFF], want.v_end[want.v_ed != 0xFF])
    assert 0.84 * m < int(want.stats[1]) < 0.88 * m  # (the probe of the reference binary: 86 % of such reads map)


def test_sharding_and_repetition_do_not_change_results(dev, c2):
    text, off, lens, bases, offs, n = c2
    whole = dev.map_batch(bases, offs, e=3)
    again = dev.map_batch(bases, offs, e=3, slot=1)
    wo, wc, we, wn = whole.per_strand()
    ao, ac, ae, an = again.per_strand()
    assert np.array_equal(wo, ao) and np.array_equal(wc, ac) and np.array_equal(we, ae) and np.array_equal(wn, an)
    h = n // 2 + 7
    lo = dev.map_batch(bases[:h * 100 + 8], offs[:h + 1], e=3)
    hi = dev.map_batch(bases[h * 100:], offs[h:] - offs[h], e=3)
    assert np.array_equal(lo.stats + hi.stats, whole.stats)
    lo_o, lo_c, lo_e, lo_n = lo.per_strand()
    hi_o, hi_c, hi_e, hi_n = hi.per_strand()
    assert np.array_equal(np.concatenate([lo_c, hi_c]), wc)
    assert np.array_equal(np.concatenate([lo_e, hi_e]), we)


def test_reverse_complementing_the_reads_swaps_the_strands(dev, c2):
    text, off, lens, bases, offs, n = c2
    m = 200_000
    fwd = bases[:m * 100].reshape(m, 100)
    comp = np.zeros(256, np.uint8)
    comp[[65, 67, 71, 84]] = [84, 71, 67, 65]
    rc = comp[fwd[:, ::-1]].reshape(-1)
    a = dev.map_batch(np.concatenate([fwd.reshape(-1), np.zeros(8, np.uint8)]), offs[:m + 1], e=3)
    b = dev.map_batch(np.concatenate([rc, np.zeros(8, np.uint8)]), offs[:m + 1], e=3)
    assert np.array_equal(a.stats, b.stats)
    ao, ac, ae, an = a.per_strand()
    bo, bc, be, bn = b.per_strand()
    ca, cb = np.diff(ao.astype(np.int64)), np.diff(bo.astype(np.int64))
    assert np.array_equal(ca[0::2], cb[1::2]) and np.array_equal(ca[1::2], cb[0::2])


def test_device_index_equals_uploaded_index_results(dev, c2):
    text, off, lens, bases, offs, n = c2
    m = 300_000
    a = dev.map_batch(bases[:m * 100 + 8], offs[:m + 1], e=3)
    n_occ, lookup, occ = dev.build_index(12, 3, fetch=True)
    dev.upload_index(12, 3, lookup, occ)
    b = dev.map_batch(bases[:m * 100 + 8], offs[:m + 1], e=3)
    assert np.array_equal(a.stats, b.stats)
    assert np.array_equal(a.per_strand()[1], b.per_strand()[1])


# ---------------------------------------------------------------------------------------------------------
# Statistical pins against the SURVEY's probe of the UNMODIFIED reference binary.
# The reference ships no vectors (the bit-exact pins are tests/test_ref_parity.py); its probe's generator and
# seeds are gone, so these are not bit-exact pins.  They compare the device path, on the same input DISTRIBUTION
# (uniform start, 0..e edits, 60/20/20 % substitution/insertion/deletion at a uniform interior offset
# of the read, truncated to L), with the counters the real binary printed.  Tolerances = 3 sigma of the probe's
# sample (binomial, for the fractions) + the rounding of the published figure + 3 sigma of ours; round 1's +-1 %
# could not tell a generator difference from a seeding bug (its generator let ~e/2L of the edits fall behind the
# truncation: P/N 3.399 against the probe's 3.362).
# ---------------------------------------------------------------------------------------------------------
def _stats(dev, text, off, lens, seed, n, L, e):
    r = dev.map_batch(*host.synth_reads(seed, text, off, lens, n, L, e, threads=16), e=e)
    N, mapped, P, C, M = [int(x) for x in r.stats]
    assert N == n and M >= mapped
    return P / N, C / N, mapped / N


def test_c2_statistics_match_the_survey_probe(dev, c2):
    # probe: 5 Mbp, 400 k reads of 100 bp, e=3: P/N = 3.362, C/N = 0.8559 (SURVEY.md 8d "[probe] per-read values")
    text, off, lens, bases, offs, n = c2
    p_n, c_n, mapped = _stats(dev, text, off, lens, 2, n, 100, 3)
    assert abs(p_n - 3.362) < 0.02, p_n
    assert abs(c_n - 0.8559) < 0.0025, c_n


def test_config1_sensitivity_profile_matches_the_survey_probe(dev):
    # probe: 1 Mbp, 1 000 reads: mapped 235/235 with 0 edits, 230/248 with 1, 206/248 with 2,
    # 170/269 with 3.  Here 200 k reads per run, split by the generator's edit count.
    text, off, lens = host.synth_reference(1, [1_000_000], threads=16)
    dev.upload_reference([text[:1_000_000]])
    dev.build_index(12, 3, fetch=False)
    n = 200_000
    n_err = np.zeros(n, np.uint8)
    bases, offs = host.synth_reads(1, text, off, lens, n, 100, 3, threads=16, n_err=n_err)
    r = dev.map_batch(bases, offs, e=3)
    o, cand, ed, end = r.per_strand()
    acc = np.add.reduceat(np.concatenate([(ed != 0xFF).astype(np.int64), [0]]), o[:-1].astype(np.int64))
    acc[np.diff(o.astype(np.int64)) == 0] = 0
    mapped = (acc[0::2] + acc[1::2]) > 0
    for k, (hit, tot) in enumerate([(235, 235), (230, 248), (206, 248), (170, 269)]):
        ours = mapped[n_err == k]
        p = hit / tot
        sigma = (p * (1 - p) / tot) ** 0.5
        assert len(ours) > 45_000
        assert abs(ours.mean() - p) <= 3 * sigma + 0.003, (k, ours.mean(), p, sigma)
    assert abs(mapped.mean() - 0.841) < 3 * (0.841 * 0.159 / 1000) ** 0.5


@pytest.fixture(scope="module")
def hg19_sized(dev):
    text, off, lens = host.synth_reference(3, [125_000_000] * 24, threads=16)
    dev.upload_reference([text[int(o):int(o) + int(l)] for o, l in zip(off, lens)])
    n_occ, _, _ = dev.build_index(12, 3, fetch=False)
    assert n_occ == 999_999_912  # index entries of the 3 Gbp / 24-sequence reference
    assert dev.seed_kernel(e=3) == "seed_join_kernel"
    return text, off, lens


def test_c3_statistics_match_the_survey_probe(dev, hg19_sized):
    # BASELINE config C3; probe: 24 x 125 Mbp, 200 k reads of 100 bp, e=3: P/N = 1 534, C/N = 0.985, 98.43 % mapped
    text, off, lens = hg19_sized
    p_n, c_n, mapped = _stats(dev, text, off, lens, 3, 1_000_000, 100, 3)
    assert abs(p_n - 1534) < 1.5, p_n
    assert abs(c_n - 0.985) < 0.0015, c_n
    assert abs(mapped - 0.9843) < 0.0012, mapped


def test_c5_statistics_match_the_survey_probe(dev, hg19_sized):
    # BASELINE config C5; probe: same reference, 100 k reads of 150 bp, e=7: P/N = 2 814, C/N = 1.002, 99.86 % mapped
    text, off, lens = hg19_sized
    assert dev.seed_kernel(e=7) == "seed_join_kernel"
    p_n, c_n, mapped = _stats(dev, text, off, lens, 5, 400_000, 150, 7)
    assert abs(p_n - 2814) < 1.5, p_n
    assert abs(c_n - 1.002) < 0.002, c_n
    assert abs(mapped - 0.9986) < 0.0006, mapped


def test_c3_c5_sharding_and_strand_symmetry_at_full_reference_size(dev, hg19_sized):
    # size-independent properties on the dense index (no oracle at 3 Gbp): a batch cut in two gives the same candidates
    # and counters; reverse-complemented reads swap their strands' candidate counts
    text, off, lens = hg19_sized
    for seed, L, e, n in ((31, 100, 3, 300_000), (51, 150, 7, 120_000)):
        bases, offs = host.synth_reads(seed, text, off, lens, n, L, e, threads=16)
        whole = dev.map_batch(bases, offs, e=e)
        h = n // 3 + 5
        lo = dev.map_batch(bases[:h * L + 8], offs[:h + 1], e=e, slot=1)
        hi = dev.map_batch(bases[h * L:], offs[h:] - offs[h], e=e, slot=2)
        assert np.array_equal(lo.stats + hi.stats, whole.stats)
        assert np.array_equal(np.concatenate([lo.per_strand()[1], hi.per_strand()[1]]), whole.per_strand()[1])
        m = 50_000
        fwd = bases[:m * L].reshape(m, L)
        comp = np.zeros(256, np.uint8)
        comp[[65, 67, 71, 84]] = [84, 71, 67, 65]
        rc = comp[fwd[:, ::-1]].reshape(-1)
        a = dev.map_batch(np.concatenate([fwd.reshape(-1), np.zeros(8, np.uint8)]), offs[:m + 1], e=e)
        b = dev.map_batch(np.concatenate([rc, np.zeros(8, np.uint8)]), offs[:m + 1], e=e)
        assert np.array_equal(a.stats, b.stats)
        ca, cb = np.diff(a.per_strand()[0].astype(np.int64)), np.diff(b.per_strand()[0].astype(np.int64))
        assert np.array_equal(ca[0::2], cb[1::2]) and np.array_equal(ca[1::2], cb[0::2])
