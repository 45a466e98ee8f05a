"""3' adapter matching on the device (fem_dev_set_adapter: adapter_match_kernel, fem_adapter.hip.h, in front of trim_clip_kernel):
the cuts against the serial rule of tests/adapter_model.py, and the as-if property of trimming with them — every array of a batch
is that of its kept parts, and its text is their text with the soft clips of tests/trim_model.py.  Needs a GPU: -m gpu."""
import functools

import numpy as np
import pytest

from fem_amd.device import FemError
from oracle import fem_oracle as fo
from tests import adapter_model as m
from tests import bam_model as bm
from tests import cases
from tests import pair_model as pm
from tests import trim_model as tm
from tests import util
from tests import xa_model as xa
from tests.harness import assert_same, assert_same_records, bam_vs_sam, device_with_env, open_device, same_text

pytestmark = pytest.mark.gpu

OFF = (0, 0, 0)
A1, A2 = m.A1, m.A2


def _q(quals):
    return np.frombuffer("".join(quals).encode("latin-1"), np.uint8)


def _map(dev, reads, rnames, quals, e, adapter=None, trim=OFF, slot=0, adapter2=None, O=m.O, E=m.E):
    """The batch staged as characters with its text, the adapter and the trims set (None: no adapter), the mapping started."""
    dev.set_trim(*trim, slot=slot)
    dev.set_adapter(adapter, adapter2, O, E, slot=slot)
    batch = fo.ReadBatch(reads)
    dev.stage_reads(batch.bases, batch.off, slot=slot)
    if adapter is not None:
        assert not dev.stage_info(slot)[1]  # as characters, whatever the lengths
    dev.stage_text(_q(quals), rnames, slot=slot)
    dev.map_staged(e=e, slot=slot)


def _check_cuts(dev, cl, a3, slot=0):
    assert [int(a) for a in dev.fetch_adapter(slot=slot)] == a3
    c5, c3 = dev.fetch_trim(slot=slot)
    assert [(int(a), int(b)) for a, b in zip(c5, c3)] == cl
    assert dev.adapter_count(slot=slot) == m.counts(a3) and dev.trim_count(slot=slot) == tm.counts(cl)


# ---- 1. the match kernel against the model ----

@pytest.fixture(scope="module")
def small_dev():
    rng = np.random.default_rng(3)
    dev = open_device([util.rand_seq(rng, 100_000)], ["chr0"])[0]
    yield dev
    dev.close()


@pytest.mark.parametrize("setting", m.SETTINGS, ids=lambda s: "O%s-E%d" % s)
@pytest.mark.parametrize("ma", m.ADAPTERS)
def test_cuts_equal_the_model_read_for_read(small_dev, ma, setting):
    full, reads, quals = m.match_case()
    assert 1500 <= len(reads) <= 2500
    A = full[:ma]
    O, E = min(setting[0] or ma, ma), setting[1]  # (the adapter of 4 letters: O = 4 for 5)
    rnames = ["c%d" % i for i in range(len(reads))]
    for trim in m.TRIMS:
        _map(small_dev, reads, rnames, quals, 3, A, trim, O=O, E=E)
        cl, a3 = m.batch_clips(reads, quals, *trim, A, O, E)
        _check_cuts(small_dev, cl, a3)
        assert m.counts(a3)[0] > 20  # the setting cuts something


def test_the_next_read_in_the_buffer_completes_no_match(small_dev):
    A = util.rand_seq(np.random.default_rng(4), 33)
    body = b"C" * 60
    reads = [body + A[:4], A[4:] + body, body[:61] + A[:3], A[3:], body + A[:20], A[20:]]
    quals = ["I" * len(r) for r in reads]
    assert m.cut_np(reads[0] + reads[1], A) == 60 + 33 and m.cut_np(reads[2] + reads[3], A) == 33  # read on, they would match
    _map(small_dev, reads, ["n%d" % i for i in range(6)], quals, 3, A)
    want = m.batch_clips(reads, quals, 0, 0, 0, A)[1]
    assert want[0] == want[2] == 0 and want[4] == 20
    assert [int(a) for a in small_dev.fetch_adapter()] == want
    _map(small_dev, reads, ["n%d" % i for i in range(6)], quals, 3, A, (0, 1, 0), O=3)  # the fixed trim moves the read's end inwards
    want = m.batch_clips(reads, quals, 0, 1, 0, A, 3)[1]
    assert want[0] == 3 and want[2] == 0 and want[4] == 19
    assert [int(a) for a in small_dev.fetch_adapter()] == want


@pytest.mark.parametrize("n", [0, 1])
def test_cuts_of_tiny_batches(small_dev, n):
    reads, quals = [b"C" * 100 + A1[:29]][:n], ["#" * 129][:n]
    _map(small_dev, reads, ["c%d" % i for i in range(n)], quals, 3, A1, (3, 4, 20))
    cl, a3 = m.batch_clips(reads, quals, 3, 4, 20, A1)
    assert (cl, a3) == ([(3, 129 - 3 - 35)][:n], [25][:n])  # a3 = 29 - 4; the quality rule takes the rest down to the floor
    _check_cuts(small_dev, cl, a3)


# ---- 2. pair mode ----

def test_mate_2_is_matched_against_its_own_adapter(small_dev):
    p = m.pairs_case()
    reads = list(p["reads"])
    planted = range(300, 340)
    for i in planted:  # mate 1's adapter inside mates 2: it must not be cut there
        reads[i] = reads[i][:50] + A1 + reads[i][83:]
    names2 = p["rnames"] + p["rnames"]
    small_dev.set_pairs(0, 500)
    try:
        _map(small_dev, reads, names2, p["quals"], 2, A1, adapter2=A2)
        cl, a3 = m.batch_clips(reads, p["quals"], 0, 0, 0, A1, A2=A2, paired=True)
        assert all(a3[i] != 70 and m.cut_np(reads[i], A1) == 70 for i in planted)
        _check_cuts(small_dev, cl, a3)
        _map(small_dev, reads, names2, p["quals"], 2, A1)  # no second adapter: the first one for both mates
        cl, a3 = m.batch_clips(reads, p["quals"], 0, 0, 0, A1, paired=True)
        assert all(a3[i] == 70 for i in planted)
        _check_cuts(small_dev, cl, a3)
    finally:
        small_dev.set_pairs(None, None)
    _map(small_dev, reads, names2, p["quals"], 2, A1, adapter2=A2)  # not in pair mode: every read is a mate 1
    cl, a3 = m.batch_clips(reads, p["quals"], 0, 0, 0, A1)
    assert all(a3[i] == 70 for i in planted)
    _check_cuts(small_dev, cl, a3)


# ---- 3. as-if on the arrays ----

@functools.lru_cache(maxsize=None)
def _oracle_kept():
    c = m.readthrough_case()
    reads, quals, cl, a3 = m.kept(c["reads"], c["quals"], 0, 0, 0, c["adapter"])
    return c, reads, quals, cl, a3, fo.map_reads(c["ref"], c["idx"], fo.ReadBatch(reads), e=c["e"], threads=8)


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_arrays_are_those_of_the_kept_parts(dense):
    c, kept_reads, kept_quals, cl, a3, want = _oracle_kept()
    assert len(set(len(r) for r in c["reads"])) == 1 and len(set(len(r) for r in kept_reads)) > 40
    dev = device_with_env(FEM_FORCE_DENSE=1) if dense else open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        if dense:
            dev.upload_reference(c["seqs"])
            dev.upload_index(12, 3, c["idx"].lookup, c["idx"].occ[:c["idx"].n_occ])
            assert dev.seed_kernel(e=c["e"]) == "seed_join_kernel"
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], c["adapter"])
        got = dev.fetch()
        assert_same(want, got)
        assert np.array_equal(dev.fetch_stats(), want.stats)
        packed = dev.fetch_packed()
        rec = dev.fetch_records()
        assert_same_records(want, rec)
        assert not np.any((rec.cigar & 15) == 4)  # the records carry no S operations
        _check_cuts(dev, cl, a3)
        _map(dev, kept_reads, c["rnames"], kept_quals, c["e"])  # the host-cut batch, no adapter, on the same handle
        plain = dev.fetch()
        for a, b in zip(got.per_strand(), plain.per_strand()):
            assert np.array_equal(a, b)
        assert np.array_equal(got.stats, plain.stats)
        plain_packed = dev.fetch_packed()
        for f in ("count", "seg_begin", "cand", "ed", "big"):
            assert np.array_equal(getattr(packed, f), getattr(plain_packed, f)), f
        assert np.array_equal(packed.end[packed.ed != 0xFF], plain_packed.end[plain_packed.ed != 0xFF])
        assert_same_records(want, dev.fetch_records())
        assert dev.adapter_count() == (0, 0) and dev.trim_count() == (0, 0)
    finally:
        dev.close()


# ---- 4. text and BAM of the read-through case ----

@pytest.fixture(scope="module")
def single():
    """The read-through case on one handle: slot 0 maps it with the adapter, slot 1 its kept parts without."""
    c, kept_reads, kept_quals, cl, a3, want = _oracle_kept()
    expect = tm.apply(cases.expected_sam(c["names"], kept_reads, c["rnames"], kept_quals, want).encode("latin-1"), c["reads"], c["quals"], cl, c["rnames"])
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], c["adapter"], slot=0)
    _map(dev, kept_reads, c["rnames"], kept_quals, c["e"], slot=1)
    yield dict(c, dev=dev, cl=cl, a3=a3, expect=expect)
    dev.close()


def _plain(dev, slot):
    dev.set_mapq(False, slot=slot), dev.set_unmapped(False, slot=slot), dev.set_report(None, None, slot=slot)
    dev.set_tags(slot=slot), dev.set_sam_seq(False, slot=slot), dev.set_xa(0, slot=slot)


def _both(s, setup):
    for slot in (0, 1):
        setup(s["dev"], slot)
    return s["dev"].fetch_sam(slot=0)[0], s["dev"].fetch_sam(slot=1)[0]


def test_text_plain_equals_the_oracle_with_the_clips(single):
    s = single
    got, base = _both(s, _plain)
    same_text(got, s["expect"])
    same_text(got, tm.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"]))
    assert len(tm.clipped_reverse_lines(got)) >= 100
    assert s["dev"].adapter_count(slot=0) == m.counts(s["a3"]) and s["dev"].trim_count(slot=0) == tm.counts(s["cl"])
    assert m.counts(s["a3"]) == tm.counts(s["cl"])  # the adapter alone: every clipped base is an adapter's


def test_text_unmapped_mapq_hits_read_group(single):
    s = single

    def setup(dev, slot):
        _plain(dev, slot)
        dev.set_unmapped(True, slot=slot), dev.set_mapq(True, slot=slot), dev.set_tags(slot=slot, read_group="grp.1", hits=True)
    got, base = _both(s, setup)
    same_text(got, tm.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"]))
    assert len(got.splitlines()) >= 600 and b"RG:Z:grp.1" in got and b"NH:i:" in got
    for slot in (0, 1):
        _plain(s["dev"], slot)


def test_text_sam_seq(single):
    s = single

    def setup(dev, slot):
        _plain(dev, slot)
        dev.set_sam_seq(True, slot=slot)
    got, base = _both(s, setup)
    same_text(got, tm.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"], sam_seq=True))
    assert got != s["expect"] and len(got) == len(s["expect"])
    for slot in (0, 1):
        _plain(s["dev"], slot)


def test_text_xa(single):
    s = single
    _plain(s["dev"], 0)
    want, n_entries = xa.apply(s["expect"], xa.ALL)
    s["dev"].set_xa(xa.ALL, slot=0)
    same_text(s["dev"].fetch_sam(slot=0)[0], want)
    assert s["dev"].xa_count(slot=0) == n_entries
    _plain(s["dev"], 0)


def test_bam_of_the_text_at_both_levels(single):
    s = single
    _plain(s["dev"], 0)
    s["dev"].set_unmapped(True, slot=0)
    ref_names = [x.encode() for x in s["names"]]
    text = bam_vs_sam(s["dev"], 0, ref_names, n_sam=1)  # levels 0 and 1 against the model's encoding of the text
    assert len(bm.records(bm.sam_to_bam_payload(text, ref_names))) == len(text.splitlines()) >= 600
    assert sum(1 for l in text.splitlines() if b"S" in l.split(b"\t")[5]) > 400
    _plain(s["dev"], 0)


# ---- 5. the pairs case ----

def _proper_share(p, text):
    """Of the pairs with a fragment below 112: the share whose two primary lines are a proper pair with TLEN = +- the fragment."""
    ok = {}
    for l in text.splitlines():
        f = l.split(b"\t")
        if not int(f[1]) & 0x100 and int(f[1]) & 2 and abs(int(f[8])) == p["frag"][int(f[0][1:])]:
            ok[int(f[0][1:])] = ok.get(int(f[0][1:]), 0) + 1
    short = [i for i in range(p["n"]) if p["frag"][i] < 112]
    return sum(1 for i in short if ok.get(i) == 2) / len(short), len(short)


def test_pairs_become_proper_pairs_with_both_adapters():
    p = m.pairs_case()
    n, names2 = p["n"], p["rnames"] + p["rnames"]
    kept_reads, kept_quals, cl, a3 = m.kept(p["reads"], p["quals"], 0, 0, 0, A1, A2=A2, paired=True)
    # the oracle with the pairing model alone, before the device is opened
    texts = []
    for reads, quals in ((kept_reads, kept_quals), (p["reads"], p["quals"])):
        res = fo.map_reads(p["ref"], p["idx"], fo.ReadBatch(reads), e=p["e"], threads=8)
        texts.append(pm.sam_lines(res, n, p["names"], reads, names2, quals, 0, 500).encode("latin-1"))
    expect = tm.apply(texts[0], p["reads"], p["quals"], cl, p["rnames"], paired=True)
    (share_on, n_short), (share_off, _) = _proper_share(p, expect), _proper_share(p, texts[1])
    print("pairs with a fragment below 112: %d; proper with TLEN = the fragment: %.3f with the adapters, %.3f without" % (n_short, share_on, share_off))
    assert n_short > 100 and share_on >= 0.90 and share_off <= 0.10
    dev = open_device(p["seqs"], p["names"], p["idx"])[0]
    try:
        dev.set_pairs(0, 500, slot=0)
        _map(dev, p["reads"], names2, p["quals"], p["e"], A1, adapter2=A2, slot=0)
        same_text(dev.fetch_sam(slot=0)[0], expect)  # pairing alone: the oracle's records through the pairing model
        for slot in (0, 1):
            dev.set_pairs(0, 500, slot=slot), dev.set_rescue(6, slot=slot), dev.set_mate_tags(True, slot=slot)
        _map(dev, p["reads"], names2, p["quals"], p["e"], A1, adapter2=A2, slot=0)
        _map(dev, kept_reads, names2, kept_quals, p["e"], slot=1)
        got, base = dev.fetch_sam(slot=0)[0], dev.fetch_sam(slot=1)[0]
        same_text(got, tm.apply(base, p["reads"], p["quals"], cl, p["rnames"], paired=True))
        assert _proper_share(p, got)[0] >= share_on  # (the rescue can only add pairs)
        assert sum(1 for l in got.splitlines() if any(x.startswith(b"MC:Z:") and b"S" in x for x in l.split(b"\t")[11:])) > 100
        _check_cuts(dev, cl, a3)
        assert dev.pair_count(slot=0) == dev.pair_count(slot=1) and dev.rescue_count(slot=0) == dev.rescue_count(slot=1)
        a, b = dev.estimate_insert(slot=0), dev.estimate_insert(slot=1)
        assert a.as_tuple() == b.as_tuple()
    finally:
        dev.close()


# ---- 6. state ----

def test_refusals_slots_and_order():
    c, kept_reads, kept_quals, cl, a3, want = _oracle_kept()
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        short = A1[:12]
        for bad in ((b"ACG", None, 3, 10), (b"A" * 65, None, 5, 10), (b"ACGTN", None, 5, 10), (A1, b"ACGU", 4, 10), (A1, b"AC", 1, 10),
                    (A1, None, 0, 10), (A1, None, 34, 10), (A1, short, 13, 10), (A1, None, 5, 31), (A1, None, 5, -1)):
            dev.set_adapter(short, None, 6, 0)
            with pytest.raises(FemError, match=r"^invalid argument: adapter"):
                dev.set_adapter(*bad)
        # ... and left the setting as it was: the first 12 letters at O = 6, E = 0 cut this batch
        _map_as_set = fo.ReadBatch(c["reads"])
        dev.stage_reads(_map_as_set.bases, _map_as_set.off)
        dev.map_staged(e=c["e"])  # the match needs no qualities: no text stage in front of the mapping
        want_short = m.batch_clips(c["reads"], c["quals"], 0, 0, 0, short, 6, 0)
        assert [int(a) for a in dev.fetch_adapter()] == want_short[1] and m.counts(want_short[1])[0] > 400
        dev.stage_text(_q(c["quals"]), c["rnames"], quals_on_host=True)
        for fetch in (dev.fetch_sam, dev.fetch_bam):  # a text with the qualities kept on the host is refused
            with pytest.raises(FemError, match=r"^invalid argument: a trimmed batch"):
                fetch()
        dev.set_trim(0, 0, 20)  # with --trim-qual the qualities must be there first, adapter or not
        dev.stage_reads(_map_as_set.bases, _map_as_set.off)
        with pytest.raises(FemError, match=r"^call order violated: quality trimming"):
            dev.map_staged(e=c["e"])
        dev.set_trim(0, 0, 0)
        # a packed batch
        from fem_amd import device
        hb, _ = dev.acquire_stage(600, 600 * 120)
        n_exc = device.pack_reads(_map_as_set.bases, 600, 120, hb)
        dev.commit_stage_packed(600, 120, n_exc)
        with pytest.raises(FemError, match=r"^input not supported by the device path: trimming"):
            dev.map_staged(e=c["e"])
        # two slots in flight with different adapters; a set_adapter between map and fetch acts on the next batch
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], A1, slot=0)
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], A1[:8], slot=1, O=8, E=0)
        dev.set_adapter(None, slot=0)
        dev.set_adapter(b"ACGTACGT", slot=1)
        _check_cuts(dev, *m.batch_clips(c["reads"], c["quals"], 0, 0, 0, A1[:8], 8, 0), slot=1)
        _check_cuts(dev, cl, a3, slot=0)
        text0 = dev.fetch_sam(slot=0)[0]
        assert len(tm.clipped_reverse_lines(text0)) >= 100
        # the adapter with set_trim off gives clips (above); with the trims on, the model's composition
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], A1, (2, 50, 20), slot=0)  # trim3 cuts most adapters' ends off
        _check_cuts(dev, *m.batch_clips(c["reads"], c["quals"], 2, 50, 20, A1), slot=0)
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], None, (0, 3, 0), slot=0)  # trimmed, but by no adapter
        with pytest.raises(FemError, match=r"^call order violated: the slot's batch was mapped without an adapter"):
            dev.fetch_adapter(slot=0)
        assert dev.adapter_count(slot=0) == (0, 0) and dev.trim_count(slot=0) == (600, 1800)
        dev.set_trim(0, 0, 0, slot=0)
        # off again: the bytes of a handle that never had an adapter
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot=0)
        off_again = dev.fetch_sam(slot=0)[0]
        with pytest.raises(FemError, match=r"^call order violated: the slot's batch was mapped without an adapter"):
            dev.fetch_adapter(slot=0)
        assert dev.adapter_count(slot=0) == (0, 0)
        fresh = open_device(c["seqs"], c["names"], c["idx"])[0]
        try:
            fresh.stage_reads(_map_as_set.bases, _map_as_set.off)
            assert fresh.stage_info()[1]  # packed, as ever
            fresh.stage_text(_q(c["quals"]), c["rnames"])
            fresh.map_staged(e=c["e"])
            assert fresh.fetch_sam()[0] == off_again
        finally:
            fresh.close()
        assert dev.stage_info(0)[1]  # the slot packed again once the adapter was off
    finally:
        dev.close()


# ---- 7. FEM map --adapter ----

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The read-through case and the pairs case as files, each beside its host-cut twin."""
    from tests.harness import build_index
    tmp = tmp_path_factory.mktemp("adapter")
    c, p = m.readthrough_case(), m.pairs_case()
    out = dict(tmp=tmp)
    for tag, case in (("s", c), ("p", p)):
        fa = tmp / (tag + ".fa")
        fa.write_bytes(b"".join(b">%s desc\n%s\n" % (n.encode(), s) for n, s in zip(case["names"], case["seqs"])))
        build_index(fa, str(tmp / (tag + ".idx")))
    kr, kq, cl, a3 = m.kept(c["reads"], c["quals"], 1, 0, 20, A1)
    cases.write_fastq(tmp / "s.fq", c["reads"], c["rnames"], c["quals"], False)
    cases.write_fastq(tmp / "s_kept.fq", kr, c["rnames"], kq, False)
    out["single"] = dict(c, cl=cl, a3=a3)
    kr, kq, cl, a3 = m.kept(p["reads"], p["quals"], 0, 0, 0, A1, A2=A2, paired=True)
    for k, half in (("1", slice(0, 300)), ("2", slice(300, 600))):
        cases.write_fastq(tmp / ("p%s.fq" % k), p["reads"][half], p["rnames"], p["quals"][half], False)
        cases.write_fastq(tmp / ("p%s_kept.fq" % k), kr[half], p["rnames"], kq[half], False)
    out["pairs"] = dict(p, cl=cl, a3=a3)
    return out


def _fem(files, tag, out, reads, *args, bam=False, e="3"):
    from tests.harness import counters, decode_bam_file, run_fem
    r = run_fem("map", "-e", e, "-t", "16", "--ref", str(files["tmp"] / (tag + ".fa")), "--index", str(files["tmp"] / (tag + ".idx")), "-o", out, *reads, *args)
    assert r.returncode == 0, r.stderr.decode()
    got = decode_bam_file(out) if bam else open(out, "rb").read()
    return b"".join(l + b"\n" for l in got.splitlines() if not l.startswith(b"@")), counters(r.stderr), r.stderr.decode()


def _split(ctr):
    own = [l for l in ctr if "trimmed" in l or "adapter" in l]
    return [l for l in ctr if l not in own], own


@pytest.mark.parametrize("batch", ["100", "100000"])
def test_cli_single_end(files, batch):
    s, tmp = files["single"], files["tmp"]
    switches = ("--adapter", A1.decode().lower(), "--trim5", "1", "--trim-qual", "20")
    opts = ("--batch", batch, "--unmapped", "--mapq")
    base, base_ctr, _ = _fem(files, "s", str(tmp / "sk.sam"), ("--read1", str(tmp / "s_kept.fq")), *opts)
    got, ctr, _ = _fem(files, "s", str(tmp / "s.sam"), ("--read1", str(tmp / "s.fq")), *opts, *switches)
    want = tm.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"])
    same_text(got, want)
    rest, own = _split(ctr)
    assert rest == base_ctr and not _split(base_ctr)[1]
    assert own == ["The number of trimmed reads: %d" % tm.counts(s["cl"])[0], "The number of trimmed bases: %d" % tm.counts(s["cl"])[1],
                   "The number of reads with adapter: %d" % m.counts(s["a3"])[0], "The number of adapter bases: %d" % m.counts(s["a3"])[1]]
    assert len(tm.clipped_reverse_lines(got)) >= 100
    if batch == "100":
        # two workers (here on one GPU): the batches are written as they retire, the lines and the summed counters are the same
        from tests.harness import counters, run_fem
        r = run_fem("map", "-e", "3", "-t", "16", "--ref", str(tmp / "s.fa"), "--index", str(tmp / "s.idx"), "-o", str(tmp / "s2.sam"), "--read1", str(tmp / "s.fq"),
                    *opts, *switches, "--gpus", "2", env=dict(FEM_TEST_SHARE_GPU="1", FEM_TESTING="1"))
        assert r.returncode == 0, r.stderr.decode()
        two = [l for l in open(str(tmp / "s2.sam"), "rb").read().splitlines() if not l.startswith(b"@")]
        assert sorted(two) == sorted(want.splitlines()) and counters(r.stderr) == ctr
        same_text(_fem(files, "s", str(tmp / "s.bam"), ("--read1", str(tmp / "s.fq")), *opts, *switches, "--bam", bam=True)[0], want)
        # the adapter alone, and the adapter off: the bytes of the run without the switch
        alone, ctr_alone, _ = _fem(files, "s", str(tmp / "sa.sam"), ("--read1", str(tmp / "s.fq")), *opts, "--adapter", A1.decode())
        cl, a3 = m.batch_clips(s["reads"], s["quals"], 0, 0, 0, A1)
        assert _split(ctr_alone)[1] == ["The number of trimmed reads: %d" % tm.counts(cl)[0], "The number of trimmed bases: %d" % tm.counts(cl)[1],
                                        "The number of reads with adapter: %d" % m.counts(a3)[0], "The number of adapter bases: %d" % m.counts(a3)[1]]
        assert tm.counts(cl) == m.counts(a3) and sum(1 for l in alone.splitlines() if not int(l.split(b"\t")[1]) & 4) > 500


def test_cli_pairs(files):
    p, tmp = files["pairs"], files["tmp"]
    switches = ("--adapter", A1.decode(), "--adapter2", A2.decode())
    opts = ("--batch", "100", "--rescue", "6", "--mate-tags", "--unmapped")
    whole = ("--read1", str(tmp / "p1.fq"), "--read2", str(tmp / "p2.fq"))
    kept = ("--read1", str(tmp / "p1_kept.fq"), "--read2", str(tmp / "p2_kept.fq"))
    base, base_ctr, _ = _fem(files, "p", str(tmp / "pk.sam"), kept, *opts, e="2")
    got, ctr, _ = _fem(files, "p", str(tmp / "p.sam"), whole, *opts, *switches, e="2")
    want = tm.apply(base, p["reads"], p["quals"], p["cl"], p["rnames"], paired=True)
    same_text(got, want)
    rest, own = _split(ctr)
    assert rest == base_ctr
    assert own == ["The number of trimmed reads: %d" % tm.counts(p["cl"])[0], "The number of trimmed bases: %d" % tm.counts(p["cl"])[1],
                   "The number of reads with adapter: %d" % m.counts(p["a3"])[0], "The number of adapter bases: %d" % m.counts(p["a3"])[1]]
    assert _proper_share(p, got)[0] >= 0.90
    same_text(_fem(files, "p", str(tmp / "p.bam"), whole, *opts, *switches, "--bam=0", bam=True, e="2")[0], want)
    # --infer-insert: the sample has its adapters cut as the run's reads have, so the learned range is the host-cut run's
    got_i, _, err = _fem(files, "p", str(tmp / "pi.sam"), whole, *opts, *switches, "--infer-insert=256", e="2")
    base_i, _, err_k = _fem(files, "p", str(tmp / "pki.sam"), kept, *opts, "--infer-insert=256", e="2")
    line = [l for l in err.splitlines() if l.startswith("Inferred insert size range")]
    assert len(line) == 1 and line == [l for l in err_k.splitlines() if l.startswith("Inferred insert size range")]
    same_text(got_i, tm.apply(base_i, p["reads"], p["quals"], p["cl"], p["rnames"], paired=True))
