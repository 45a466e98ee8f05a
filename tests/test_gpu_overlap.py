"""The mates' overlap on the device (fem_dev_set_pair_overlap: pair_overlap_kernel, fem_overlap.hip.h, in front of
trim_clip_kernel): the cuts against the rule of tests/overlap_model.py pair for pair, and the as-if property of trimming with
them — every array of a batch is that of its kept parts, and its text is their text with the soft clips of tests/trim_model.py.
Needs a GPU: -m gpu."""
import functools

import numpy as np
import pytest

from fem_amd.device import FemError
from oracle import fem_oracle as fo
from tests import adapter_model as am
from tests import bam_model as bm
from tests import cases
from tests import overlap_model as m
from tests import pair_model as pm
from tests import trim_model as tm
from tests import util
from tests.harness import assert_same, assert_same_records, bam_vs_sam, device_with_env, open_device, same_text

pytestmark = pytest.mark.gpu

OFF = (0, 0, 0)
A1, A2 = am.A1, am.A2


def _q(quals):
    return np.frombuffer("".join(quals).encode("latin-1"), np.uint8)


def _map(dev, reads, rnames, quals, e, overlap=(m.O, m.E), trim=OFF, slot=0, adapter=None, adapter2=None):
    """The batch of pairs staged as characters with its text, the overlap (None: off), the adapter and the trims set, the
    mapping started.  The slot's pair mode is the caller's."""
    dev.set_trim(*trim, slot=slot)
    dev.set_adapter(adapter, adapter2, slot=slot)
    if overlap is None:
        dev.set_pair_overlap(None, slot=slot)
    else:
        dev.set_pair_overlap(*overlap, slot=slot)
    batch = fo.ReadBatch(reads)
    dev.stage_reads(batch.bases, batch.off, slot=slot)
    if overlap is not None:
        assert not dev.stage_info(slot)[1]  # as characters, whatever the lengths
    dev.stage_text(_q(quals), rnames, slot=slot)
    dev.map_staged(e=e, slot=slot)


def _check_cuts(dev, cl, v3, slot=0):
    assert [int(a) for a in dev.fetch_pair_overlap(slot=slot)] == v3
    c5, c3 = dev.fetch_trim(slot=slot)
    assert [(int(a), int(b)) for a, b in zip(c5, c3)] == cl
    assert dev.pair_overlap_count(slot=slot) == m.counts(v3) and dev.trim_count(slot=slot) == tm.counts(cl)


def _names2(n):
    return ["c%d" % i for i in range(n)] * 2


# ---- 1. the kernel against the model ----

@pytest.fixture(scope="module")
def small_dev():
    rng = np.random.default_rng(3)
    dev = open_device([util.rand_seq(rng, 100_000)], ["chr0"])[0]
    dev.set_pairs(0, 500)
    yield dev
    dev.close()


@pytest.mark.parametrize("setting", m.SETTINGS, ids=lambda s: "O%d-E%d" % s)
def test_cuts_equal_the_model_pair_for_pair(small_dev, setting):
    reads, quals = m.match_case()
    n = len(reads) // 2
    assert 1300 <= n <= 1700
    for trim in m.TRIMS:
        _map(small_dev, reads, _names2(n), quals, 3, setting, trim)
        cl, v3, _ = m.batch_clips(reads, quals, *trim, *setting)
        _check_cuts(small_dev, cl, v3)
        assert (m.counts(v3)[0] > 300) == (setting[0] != 1024)  # the setting cuts something; the last one cannot
        with pytest.raises(FemError, match=r"^call order violated: the slot's batch was mapped without an adapter"):
            small_dev.fetch_adapter()
        assert small_dev.adapter_count() == (0, 0)


def test_the_next_read_in_the_buffer_completes_no_match(small_dev):
    rng = np.random.default_rng(4)
    fragment, rest = util.rand_seq(rng, 40), util.rand_seq(rng, 30)
    # pair 0: mate 1 holds 15 bases of the fragment only, the read behind it in the buffer the other 25; pair 2 the same for mate 2
    m1 = [fragment[:15], fragment[15:] + rest, (fragment + rest)[:60], util.rand_seq(rng, 50)]
    m2 = [(util.revcomp(fragment) + rest)[:60], util.rand_seq(rng, 50), util.revcomp(fragment)[:15], util.revcomp(fragment)[15:] + rest]
    reads = m1 + m2
    quals = ["I" * len(r) for r in reads]
    assert m.frag_np(m1[0] + m1[1], m2[0]) == 40 and m.frag_np(m1[2], m2[2] + m2[3]) == 40  # read on, they would match
    _map(small_dev, reads, _names2(4), quals, 3)
    cl, v3, _ = m.batch_clips(reads, quals, 0, 0, 0)
    assert v3 == [0] * 8
    _check_cuts(small_dev, cl, v3)
    _map(small_dev, reads, _names2(4), quals, 3, (12, 0), (0, 2, 0))  # 13 bases overlap behind the fixed trim: a match of its own
    cl, v3, _ = m.batch_clips(reads, quals, 0, 2, 0, 12, 0)
    assert v3[0] == 0 and v3[4] == 58 - 40 and v3[2] == 58 - 40 and v3[6] == 0
    _check_cuts(small_dev, cl, v3)


@pytest.mark.parametrize("n", [0, 1])
def test_cuts_of_tiny_batches(small_dev, n):
    fragment = util.rand_seq(np.random.default_rng(5), 80)
    reads = ([fragment + b"ACGTACGTAC"] * n) + ([util.revcomp(fragment) + b"CCCCCCCCCCCCCCC"] * n)
    quals = (["I" * 60 + "#" * 30] * n) + (["I" * 95] * n)
    _map(small_dev, reads, _names2(n), quals, 3, trim=(3, 4, 20))
    cl, v3, _ = m.batch_clips(reads, quals, 3, 4, 20)
    assert (cl, v3) == ([(3, 4 + 9 + 17), (3, 4 + 14)][:2 * n], [9, 14][:2 * n])  # the fragment behind the trims is 74 bases; its 17 bad ones go too
    _check_cuts(small_dev, cl, v3)


def test_adapter_and_overlap_together_take_the_larger_cut(small_dev):
    p = am.pairs_case()
    reads = list(p["reads"])
    for i in range(40):  # mate 1's adapter planted inside the fragment of mates 1: there the adapter's cut is the larger
        reads[i] = reads[i][:50] + A1 + reads[i][83:]
    names2 = p["rnames"] + p["rnames"]
    _map(small_dev, reads, names2, p["quals"], 2, adapter=A1, adapter2=A2, trim=(0, 0, 20))
    cl, v3, a3 = m.batch_clips(reads, p["quals"], 0, 0, 20, A=A1, A2=A2)
    assert sum(1 for a, v in zip(a3, v3) if a > v) >= 40 and sum(1 for a, v in zip(a3, v3) if v > a) >= 10
    assert [c3 for _, c3 in cl] == [max(a, v) for a, v in zip(a3, v3)]  # (the qualities are good: the quality rule adds nothing)
    _check_cuts(small_dev, cl, v3)
    assert [int(a) for a in small_dev.fetch_adapter()] == a3 and small_dev.adapter_count() == am.counts(a3)  # the adapter's own matches


def test_fetches_repeat_and_end_with_their_batch(small_dev):
    """Every producer's cuts come home once per batch: a second fetch gives what the first gave, and the slot's next batch, the
    same pairs in reverse order, gives its own."""
    p = am.pairs_case()
    n, names2, seen = p["n"], p["rnames"] + p["rnames"], []
    for pairs in (list(range(n)), list(range(n - 1, -1, -1))):
        pick = pairs + [n + i for i in pairs]
        reads, quals = [p["reads"][i] for i in pick], [p["quals"][i] for i in pick]
        _map(small_dev, reads, [names2[i] for i in pick], quals, 2, adapter=A1, adapter2=A2, trim=(2, 3, 20))
        cl, v3, a3 = m.batch_clips(reads, quals, 2, 3, 20, A=A1, A2=A2)
        assert m.counts(v3)[0] > 100 and am.counts(a3)[0] > 100 and all(c5 == 2 and c3 >= 3 for c5, c3 in cl)
        for _ in range(2):
            _check_cuts(small_dev, cl, v3)
            assert [int(a) for a in small_dev.fetch_adapter()] == a3 and small_dev.adapter_count() == am.counts(a3)
        seen.append((cl, v3, a3))
    assert all(a != b for a, b in zip(*seen))  # an array left over from the first batch would not pass for the second's


# ---- 2. as-if on the arrays and in the text: the pairs case ----

@functools.lru_cache(maxsize=None)
def _oracle_kept():
    p = am.pairs_case()
    reads, quals, cl, v3, _ = m.kept(p["reads"], p["quals"], 0, 0, 0)
    return p, reads, quals, cl, v3, fo.map_reads(p["ref"], p["idx"], fo.ReadBatch(reads), e=p["e"], threads=8)


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_arrays_are_those_of_the_kept_parts(dense):
    p, kept_reads, kept_quals, cl, v3, want = _oracle_kept()
    names2 = p["rnames"] + p["rnames"]
    assert len(set(len(r) for r in p["reads"])) == 1 and len(set(len(r) for r in kept_reads)) > 40
    dev = device_with_env(FEM_FORCE_DENSE=1) if dense else open_device(p["seqs"], p["names"], p["idx"])[0]
    try:
        if dense:
            dev.upload_reference(p["seqs"])
            dev.upload_index(12, 3, p["idx"].lookup, p["idx"].occ[:p["idx"].n_occ])
            assert dev.seed_kernel(e=p["e"]) == "seed_join_kernel"
        dev.set_pairs(0, 500)
        _map(dev, p["reads"], names2, p["quals"], p["e"])
        got = dev.fetch()
        assert_same(want, got)
        assert np.array_equal(dev.fetch_stats(), want.stats)
        packed = dev.fetch_packed()
        rec = dev.fetch_records()
        assert_same_records(want, rec)
        assert not np.any((rec.cigar & 15) == 4)  # the records carry no S operations
        _check_cuts(dev, cl, v3)
        _map(dev, kept_reads, names2, kept_quals, p["e"], None)  # the host-cut batch, no overlap, on the same handle
        plain = dev.fetch()
        for a, b in zip(got.per_strand(), plain.per_strand()):
            assert np.array_equal(a, b)
        assert np.array_equal(got.stats, plain.stats)
        plain_packed = dev.fetch_packed()
        for f in ("count", "seg_begin", "cand", "ed", "big"):
            assert np.array_equal(getattr(packed, f), getattr(plain_packed, f)), f
        assert np.array_equal(packed.end[packed.ed != 0xFF], plain_packed.end[plain_packed.ed != 0xFF])
        assert_same_records(want, dev.fetch_records())
        assert dev.pair_overlap_count() == (0, 0) and dev.trim_count() == (0, 0)
    finally:
        dev.close()


def _proper(p, text):
    """The pairs whose two primary lines are a proper pair with TLEN = +- the fragment."""
    ok = {}
    for l in text.splitlines():
        f = l.split(b"\t")
        if not int(f[1]) & 0x100 and int(f[1]) & 2 and abs(int(f[8])) == p["frag"][int(f[0][1:])]:
            ok[int(f[0][1:])] = ok.get(int(f[0][1:]), 0) + 1
    return set(i for i, k in ok.items() if k == 2)


def _proper_share(p, text):
    """Of the pairs with a fragment below 112: the share that _proper holds."""
    short = [i for i in range(p["n"]) if p["frag"][i] < 112]
    return len(_proper(p, text) & set(short)) / len(short), len(short)


def test_pairs_become_proper_pairs_with_the_overlap_alone():
    p, kept_reads, kept_quals, cl, v3, want = _oracle_kept()
    n, names2 = p["n"], p["rnames"] + p["rnames"]
    # the oracle with the pairing model alone, before the device is opened: the overlap's cut, the adapters' cut, no cut
    ad_reads, ad_quals, ad_cl, ad_a3 = am.kept(p["reads"], p["quals"], 0, 0, 0, A1, A2=A2, paired=True)
    texts = [pm.sam_lines(want, n, p["names"], kept_reads, names2, kept_quals, 0, 500).encode("latin-1")]
    for reads, quals in ((ad_reads, ad_quals), (p["reads"], p["quals"])):
        res = fo.map_reads(p["ref"], p["idx"], fo.ReadBatch(reads), e=p["e"], threads=8)
        texts.append(pm.sam_lines(res, n, p["names"], reads, names2, quals, 0, 500).encode("latin-1"))
    expect = tm.apply(texts[0], p["reads"], p["quals"], cl, p["rnames"], paired=True)
    (share_on, n_short), (share_off, _) = _proper_share(p, expect), _proper_share(p, texts[2])
    below = set(i for i in range(n) if p["frag"][i] < 120)
    print("pairs with a fragment below 112: %d; proper with TLEN = the fragment: %.3f with the overlap, %.3f without" % (n_short, share_on, share_off))
    print("of the %d pairs with a fragment below 120, proper pairs with TLEN = the fragment: %d with --trim-overlap alone, %d with --adapter "
          "and --adapter2 alone, %d with neither" % (len(below), len(_proper(p, expect) & below), len(_proper(p, texts[1]) & below), len(_proper(p, texts[2]) & below)))
    assert n_short > 100 and share_on >= 0.90 and share_off <= 0.10
    # a read-through of 1 to 4 bases: the overlap cuts it, the adapter at its default overlap leaves it
    few = [i for i in range(n) if 116 <= p["frag"][i] <= 119]
    assert len(few) >= 5 and all(v3[i] == v3[n + i] == 120 - p["frag"][i] for i in few)
    dev = open_device(p["seqs"], p["names"], p["idx"])[0]
    try:
        dev.set_pairs(0, 500, slot=0)
        _map(dev, p["reads"], names2, p["quals"], p["e"], None, adapter=A1, adapter2=A2, slot=0)  # --adapter alone
        a3 = dev.fetch_adapter(slot=0)
        assert all(int(a3[i]) == 0 and int(a3[n + i]) == 0 for i in few) and [int(a) for a in a3] == ad_a3
        _map(dev, p["reads"], names2, p["quals"], p["e"], slot=0)
        got_v3 = dev.fetch_pair_overlap(slot=0)
        assert all(int(got_v3[i]) == int(got_v3[n + i]) == 120 - p["frag"][i] for i in few)
        plain = dev.fetch_sam(slot=0)[0]
        same_text(plain, expect)  # pairing alone: the oracle's records through the pairing model
        assert _proper_share(p, plain)[0] >= share_on
        ref_names = [x.encode() for x in p["names"]]
        bam_vs_sam(dev, 0, ref_names, n_sam=1)  # BAM at levels 0 and 1 against the model's encoding of the text
        for slot in (0, 1):
            dev.set_pairs(0, 500, slot=slot), dev.set_rescue(6, slot=slot), dev.set_mate_tags(True, slot=slot)
        _map(dev, p["reads"], names2, p["quals"], p["e"], slot=0)
        _map(dev, kept_reads, names2, kept_quals, p["e"], None, slot=1)
        got, base = dev.fetch_sam(slot=0)[0], dev.fetch_sam(slot=1)[0]
        same_text(got, tm.apply(base, p["reads"], p["quals"], cl, p["rnames"], paired=True))
        assert _proper_share(p, got)[0] >= share_on  # (the rescue can only add pairs)
        assert sum(1 for l in got.splitlines() if any(x.startswith(b"MC:Z:") and b"S" in x for x in l.split(b"\t")[11:])) > 100
        for level in (0, 1):  # (the mate tags' records decode to their lines: ms is an I in the record, which the model's encoder does not write)
            data, raw_len = dev.fetch_bam(slot=0, level=level)[:2]
            payload = b"".join(x[0] for x in bm.parse_bgzf(data, eof=False))
            assert raw_len == len(payload) and bm.bam_payload_to_sam(payload, ref_names) == got
            assert len(bm.records(payload)) == len(got.splitlines()) >= 500
        _check_cuts(dev, cl, v3)
        assert dev.pair_count(slot=0) == dev.pair_count(slot=1) and dev.rescue_count(slot=0) == dev.rescue_count(slot=1)
        a, b = dev.estimate_insert(slot=0), dev.estimate_insert(slot=1)
        assert a.as_tuple() == b.as_tuple()
        # the overlap is the sequencer's geometry: the same cuts under another orientation
        dev.set_orientation("rf", slot=0)
        _map(dev, p["reads"], names2, p["quals"], p["e"], slot=0)
        _check_cuts(dev, cl, v3)
    finally:
        dev.close()


# ---- 3. state ----

def test_refusals_slots_and_order():
    p, kept_reads, kept_quals, cl, v3, want = _oracle_kept()
    names2 = p["rnames"] + p["rnames"]
    dev = open_device(p["seqs"], p["names"], p["idx"])[0]
    try:
        dev.set_pairs(0, 500, slot=0), dev.set_pairs(0, 500, slot=1)
        for bad in ((7, 10), (1025, 10), (0, 10), (-1, 10), (20, 31), (20, -1)):
            dev.set_pair_overlap(30, 0)
            with pytest.raises(FemError, match=r"^invalid argument: pair overlap"):
                dev.set_pair_overlap(*bad)
        # ... and left the setting as it was: O = 30, E = 0 cut this batch
        batch = fo.ReadBatch(p["reads"])
        dev.stage_reads(batch.bases, batch.off)
        dev.map_staged(e=p["e"])  # the match needs no qualities: no text stage in front of the mapping
        want_30 = m.batch_clips(p["reads"], p["quals"], 0, 0, 0, 30, 0)
        assert [int(a) for a in dev.fetch_pair_overlap()] == want_30[1] and m.counts(want_30[1])[0] == 160
        # not in pair mode
        dev.set_pairs(None, None)
        dev.stage_reads(batch.bases, batch.off)
        with pytest.raises(FemError, match=r"^call order violated: the mates' overlap"):
            dev.map_staged(e=p["e"])
        dev.set_pairs(0, 500)
        # a packed batch
        from fem_amd import device
        hb, _ = dev.acquire_stage(600, 600 * 120)
        n_exc = device.pack_reads(batch.bases, 600, 120, hb)
        dev.commit_stage_packed(600, 120, n_exc)
        with pytest.raises(FemError, match=r"^input not supported by the device path: trimming"):
            dev.map_staged(e=p["e"])
        # two slots in flight with different settings; a set between map and fetch acts on the next batch
        _map(dev, p["reads"], names2, p["quals"], p["e"], slot=0)
        _map(dev, p["reads"], names2, p["quals"], p["e"], (100, 0), slot=1)
        dev.set_pair_overlap(None, slot=0)
        dev.set_pair_overlap(8, 30, slot=1)
        cl_100, v3_100, _ = m.batch_clips(p["reads"], p["quals"], 0, 0, 0, 100, 0)
        assert 0 < m.counts(v3_100)[0] < 100
        _check_cuts(dev, cl_100, v3_100, slot=1)
        _check_cuts(dev, cl, v3, slot=0)
        text0 = dev.fetch_sam(slot=0)[0]
        assert len(tm.clipped_reverse_lines(text0)) >= 100
        # mapped without the setting, trimmed or not: the fetch is refused, the counts are 0
        _map(dev, p["reads"], names2, p["quals"], p["e"], None, (0, 3, 0), slot=0)
        with pytest.raises(FemError, match=r"^call order violated: the slot's batch was mapped without the mates' overlap"):
            dev.fetch_pair_overlap(slot=0)
        assert dev.pair_overlap_count(slot=0) == (0, 0) and dev.trim_count(slot=0) == (600, 1800)
        # off again: the bytes of a handle that never had the setting
        _map(dev, p["reads"], names2, p["quals"], p["e"], None, slot=0)
        off_again = dev.fetch_sam(slot=0)[0]
        with pytest.raises(FemError, match=r"^call order violated: the slot's batch was mapped without the mates' overlap"):
            dev.fetch_pair_overlap(slot=0)
        assert dev.pair_overlap_count(slot=0) == (0, 0)
        fresh = open_device(p["seqs"], p["names"], p["idx"])[0]
        try:
            fresh.set_pairs(0, 500)
            fresh.stage_reads(batch.bases, batch.off)
            assert fresh.stage_info()[1]  # packed, as ever
            fresh.stage_text(_q(p["quals"]), names2)
            fresh.map_staged(e=p["e"])
            assert fresh.fetch_sam()[0] == off_again
        finally:
            fresh.close()
        assert dev.stage_info(0)[1]  # the slot packed again once the setting was off
    finally:
        dev.close()


# ---- 4. FEM map --trim-overlap ----

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The pairs case as files beside its host-cut twins: cut by the overlap alone, and by the overlap and the adapters."""
    from tests.harness import build_index
    tmp = tmp_path_factory.mktemp("overlap")
    p = am.pairs_case()
    fa = tmp / "p.fa"
    fa.write_bytes(b"".join(b">%s desc\n%s\n" % (n.encode(), s) for n, s in zip(p["names"], p["seqs"])))
    build_index(fa, str(tmp / "p.idx"))
    out = dict(p, tmp=tmp)
    for tag, kw in (("kept", {}), ("both", dict(A=A1, A2=A2))):
        kr, kq, cl, v3, a3 = m.kept(p["reads"], p["quals"], 0, 0, 0, **kw)
        for k, half in (("1", slice(0, 300)), ("2", slice(300, 600))):
            cases.write_fastq(tmp / ("p%s_%s.fq" % (k, tag)), kr[half], p["rnames"], kq[half], False)
        out[tag] = dict(cl=cl, v3=v3, a3=a3)
    for k, half in (("1", slice(0, 300)), ("2", slice(300, 600))):
        cases.write_fastq(tmp / ("p%s.fq" % k), p["reads"][half], p["rnames"], p["quals"][half], False)
    return out


def _fem(files, out, reads, *args, bam=False, env=None):
    from tests.harness import counters, decode_bam_file, run_fem
    r = run_fem("map", "-e", "2", "-t", "16", "--ref", str(files["tmp"] / "p.fa"), "--index", str(files["tmp"] / "p.idx"), "-o", out, *reads, *args, env=env)
    assert r.returncode == 0, r.stderr.decode()
    got = decode_bam_file(out) if bam else open(out, "rb").read()
    return b"".join(l + b"\n" for l in got.splitlines() if not l.startswith(b"@")), counters(r.stderr), r.stderr.decode()


def _split(ctr):
    own = [l for l in ctr if "trimmed" in l or "adapter" in l or "overlap" in l]
    return [l for l in ctr if l not in own], own


def _reads(files, tag=None):
    tmp = files["tmp"]
    return ("--read1", str(tmp / ("p1_%s.fq" % tag if tag else "p1.fq")), "--read2", str(tmp / ("p2_%s.fq" % tag if tag else "p2.fq")))


def _own_lines(k):
    return ["The number of trimmed reads: %d" % tm.counts(k["cl"])[0], "The number of trimmed bases: %d" % tm.counts(k["cl"])[1],
            "The number of pairs with overlap cut: %d" % m.counts(k["v3"])[0], "The number of overlap bases: %d" % m.counts(k["v3"])[1]]


def test_cli_pairs(files):
    p, tmp, k = files, files["tmp"], files["kept"]
    opts = ("--batch", "100", "--rescue", "6", "--mate-tags", "--unmapped")
    base, base_ctr, _ = _fem(files, str(tmp / "pk.sam"), _reads(files, "kept"), *opts)
    got, ctr, _ = _fem(files, str(tmp / "p.sam"), _reads(files), *opts, "--trim-overlap")
    want = tm.apply(base, p["reads"], p["quals"], k["cl"], p["rnames"], paired=True)
    same_text(got, want)
    rest, own = _split(ctr)
    assert rest == base_ctr and not _split(base_ctr)[1]
    assert own == _own_lines(k) and m.counts(k["v3"]) == (160, tm.counts(k["cl"])[1])  # the overlap alone: every clipped base is its own
    assert _proper_share(p, got)[0] >= 0.90
    same_text(_fem(files, str(tmp / "p.bam"), _reads(files), *opts, "--trim-overlap", "--bam=0", bam=True)[0], want)
    # two workers (here on one GPU): the batches are written as they retire, the lines and the summed counters are the same
    two, ctr2, _ = _fem(files, str(tmp / "p2.sam"), _reads(files), *opts, "--trim-overlap", "--gpus", "2", env=dict(FEM_TEST_SHARE_GPU="1", FEM_TESTING="1"))
    assert sorted(two.splitlines()) == sorted(want.splitlines()) and ctr2 == ctr
    # the defaults spelled out, and another orientation: the same cuts
    _, ctr_d, _ = _fem(files, str(tmp / "pd.sam"), _reads(files), *opts, "--trim-overlap", "--trim-overlap-min", "20", "--trim-overlap-err", "10")
    assert ctr_d == ctr
    _, ctr_rf, _ = _fem(files, str(tmp / "prf.sam"), _reads(files), *opts, "--trim-overlap", "--orientation", "rf")
    assert _split(ctr_rf)[1] == own


def test_cli_infer_insert_and_adapters(files):
    p, tmp, k, both = files, files["tmp"], files["kept"], files["both"]
    opts = ("--batch", "100", "--rescue", "6", "--mate-tags", "--unmapped")
    # --infer-insert: the sample is cut as the run's reads are, so the learned range is the host-cut run's
    got_i, _, err = _fem(files, str(tmp / "pi.sam"), _reads(files), *opts, "--trim-overlap", "--infer-insert=256")
    base_i, _, err_k = _fem(files, str(tmp / "pki.sam"), _reads(files, "kept"), *opts, "--infer-insert=256")
    line = [l for l in err.splitlines() if l.startswith("Inferred insert size range")]
    assert len(line) == 1 and line == [l for l in err_k.splitlines() if l.startswith("Inferred insert size range")]
    same_text(got_i, tm.apply(base_i, p["reads"], p["quals"], k["cl"], p["rnames"], paired=True))
    # together with --adapter / --adapter2: the larger cut, every cut base counted once, the adapter's lines its own matches
    base, base_ctr, _ = _fem(files, str(tmp / "pb.sam"), _reads(files, "both"), *opts)
    got, ctr, _ = _fem(files, str(tmp / "pa.sam"), _reads(files), *opts, "--trim-overlap", "--adapter", A1.decode(), "--adapter2", A2.decode())
    same_text(got, tm.apply(base, p["reads"], p["quals"], both["cl"], p["rnames"], paired=True))
    rest, own = _split(ctr)
    assert rest == base_ctr
    assert own == _own_lines(both)[:2] + ["The number of reads with adapter: %d" % am.counts(both["a3"])[0],
                                          "The number of adapter bases: %d" % am.counts(both["a3"])[1]] + _own_lines(both)[2:]
    assert tm.counts(both["cl"])[1] == sum(max(a, v) for a, v in zip(both["a3"], both["v3"]))
