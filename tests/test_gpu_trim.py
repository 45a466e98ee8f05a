"""Read trimming on the device (fem_dev_set_trim: trim_clip_kernel and trim_gather_kernel, fem_trim.hip.h; the clip stage of the
text, fem_tail.hip): the clip points against the serial rule of tests/trim_model.py, and the as-if property — every array of a
trimmed batch is the array of the batch of the kept parts, and its text is that batch's text with the model's differences.
Needs a GPU: -m gpu."""
import functools

import numpy as np
import pytest

from fem_amd.device import FemError
from oracle import fem_oracle as fo
from tests import bam_model as bm
from tests import cases
from tests import mate_tags_model as mt
from tests import trim_model as m
from tests import util
from tests import xa_model as xa
from tests.cases import I, X
from tests.harness import assert_same, assert_same_records, bam_vs_sam, device_with_env, open_device, same_text

pytestmark = pytest.mark.gpu

OFF = (0, 0, 0)


def _q(quals):
    return np.frombuffer("".join(quals).encode("latin-1"), np.uint8)


def _map(dev, reads, rnames, quals, e, trim, slot=0):
    """The batch staged as characters with its text, trimming set to `trim`, the mapping started."""
    dev.set_trim(*trim, slot=slot)
    batch = fo.ReadBatch(reads)
    dev.stage_reads(batch.bases, batch.off, slot=slot)
    if trim != OFF:
        assert not dev.stage_info(slot)[1]  # as characters, whatever the lengths
    dev.stage_text(_q(quals), rnames, slot=slot)
    dev.map_staged(e=e, slot=slot)


def _kept(c, trim=None):
    return m.kept(c["reads"], c["quals"], *(trim or c["trim"]))


# ---- 1. the clip kernel against the model ----

@pytest.fixture(scope="module")
def small_dev():
    rng = np.random.default_rng(3)
    dev = open_device([util.rand_seq(rng, 100_000)], ["chr0"])[0]
    yield dev
    dev.close()


@pytest.mark.parametrize("trim", m.SETTINGS, ids=lambda t: "%d-%d-%d" % t)
def test_clip_points_equal_the_model_read_for_read(small_dev, trim):
    reads, quals = m.clip_case()
    assert 1900 <= len(reads) <= 2100
    _map(small_dev, reads, ["c%d" % i for i in range(len(reads))], quals, 3, trim)
    want = m.batch_clips(quals, *trim)
    c5, c3 = small_dev.fetch_trim()
    assert [(int(a), int(b)) for a, b in zip(c5, c3)] == want
    assert small_dev.trim_count() == m.counts(want)
    assert m.counts(want)[0] > 100  # the setting cuts something


@pytest.mark.parametrize("n", [0, 1])
def test_clip_points_of_tiny_batches(small_dev, n):
    reads, quals = m.clip_case()
    k = next(i for i, r in enumerate(reads) if len(r) == 129 and set(quals[i]) == {"#"})
    reads, quals = reads[k:k + n], quals[k:k + n]
    _map(small_dev, reads, ["c%d" % i for i in range(n)], quals, 3, (3, 4, 20))
    want = m.batch_clips(quals, 3, 4, 20)
    c5, c3 = small_dev.fetch_trim()
    assert [(int(a), int(b)) for a, b in zip(c5, c3)] == want == [(3, 129 - 3 - 35)][:n]
    assert small_dev.trim_count() == m.counts(want)


# ---- 2. as-if on the arrays ----

def _case(name):
    """A case of the model, on both index forms as it is: with the reads whose kept part is empty."""
    return getattr(m, name)()


@functools.lru_cache(maxsize=None)
def _oracle_kept(name):
    c = _case(name)
    reads, quals, cl = _kept(c)
    return reads, quals, cl, fo.map_reads(c["ref"], c["idx"], fo.ReadBatch(reads), e=c["e"], threads=8)


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("name", ["tails_case", "ragged_case"])
def test_arrays_are_those_of_the_kept_parts(name, dense):
    c = _case(name)
    kept_reads, kept_quals, cl, want = _oracle_kept(name)
    assert min(len(r) for r in kept_reads) == (0 if name == "ragged_case" else 80)
    if name == "ragged_case":  # a read of no bases, and one the fixed trims use up: on the dense index too
        assert len(c["reads"][7]) == 0 and len(c["reads"][11]) == 6 and len(kept_reads[7]) == len(kept_reads[11]) == 0
    assert (len(set(len(r) for r in c["reads"])) == 1) == (name == "tails_case")  # equal lengths through stage_reads, and ragged
    dev = device_with_env(FEM_FORCE_DENSE=1) if dense else open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        if dense:
            dev.upload_reference(c["seqs"])
            dev.upload_index(12, 3, c["idx"].lookup, c["idx"].occ[:c["idx"].n_occ])
            assert dev.seed_kernel(e=c["e"]) == "seed_join_kernel"
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], c["trim"])
        got = dev.fetch()
        assert_same(want, got)
        assert np.array_equal(dev.fetch_stats(), want.stats)
        packed = dev.fetch_packed()
        rec = dev.fetch_records()
        assert_same_records(want, rec)
        assert not np.any((rec.cigar & 15) == 4)  # the records carry no S operations
        _map(dev, kept_reads, c["rnames"], kept_quals, c["e"], OFF)  # the host-trimmed batch, trimming off, on the same handle
        plain = dev.fetch()
        for a, b in zip(got.per_strand(), plain.per_strand()):
            assert np.array_equal(a, b)
        assert np.array_equal(got.stats, plain.stats)
        plain_packed = dev.fetch_packed()
        for f in ("count", "seg_begin", "cand", "ed", "big"):
            assert np.array_equal(getattr(packed, f), getattr(plain_packed, f)), f
        assert np.array_equal(packed.end[packed.ed != 0xFF], plain_packed.end[plain_packed.ed != 0xFF])
        assert_same_records(want, dev.fetch_records())
        assert dev.trim_count() == (0, 0)
    finally:
        dev.close()


# ---- 3. the tails case ----

def _mapped_names(text):
    return set(l.split(b"\t", 1)[0] for l in text.splitlines())


def test_tails_map_with_the_switch_and_not_without():
    c = m.tails_case()
    kept_reads, kept_quals, cl, want = _oracle_kept("tails_case")
    assert [b for a, b in cl] == c["tails"] and all(a == 0 for a, b in cl)  # the cut is the tail's start by construction
    long_tail = [c["rnames"][i].encode() for i, t in enumerate(c["tails"]) if t >= 8]
    assert len(long_tail) >= 400
    # the oracle on its own inputs: the whole reads, and the kept parts
    whole = fo.map_reads(c["ref"], c["idx"], fo.ReadBatch(c["reads"]), e=c["e"], threads=8)
    as_given = cases.expected_sam(c["names"], c["reads"], c["rnames"], c["quals"], whole).encode("latin-1")
    kept_text = cases.expected_sam(c["names"], kept_reads, c["rnames"], kept_quals, want).encode("latin-1")
    expect = m.apply(kept_text, c["reads"], c["quals"], cl, c["rnames"])
    with_switch, without = _mapped_names(expect), _mapped_names(as_given)
    share_on = sum(1 for n in long_tail if n in with_switch) / len(long_tail)
    share_off = sum(1 for n in long_tail if n in without) / len(long_tail)
    print("reads with a tail >= 8: %d; with a line: %.3f with the switch, %.3f without" % (len(long_tail), share_on, share_off))
    assert share_on >= 0.90 and share_off <= 0.10
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], c["trim"])
        text = dev.fetch_sam()[0]
        same_text(text, expect)
        assert len(m.clipped_reverse_lines(text)) >= 100
        assert dev.trim_count() == m.counts(cl)
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], OFF)
        same_text(dev.fetch_sam()[0], as_given)
    finally:
        dev.close()


# ---- 4. text and BAM, single-end ----

@pytest.fixture(scope="module")
def single():
    """ragged_case on a repeat-rich reference on one handle: slot 0 maps the trimmed batch, slot 1 the kept parts, trimming off."""
    c = m.ragged_case(True)
    kept_reads, kept_quals, cl = _kept(c)
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], c["trim"], slot=0)
    _map(dev, kept_reads, c["rnames"], kept_quals, c["e"], OFF, slot=1)
    yield dict(c, dev=dev, cl=cl)
    dev.close()


def _both(s, setup):
    """The two slots' texts under the same line options -> (the trimmed batch's, the kept parts')."""
    for slot in (0, 1):
        setup(s["dev"], slot)
    return s["dev"].fetch_sam(slot=0)[0], s["dev"].fetch_sam(slot=1)[0]


def _plain(dev, slot):
    dev.set_mapq(False, slot=slot), dev.set_unmapped(False, slot=slot), dev.set_report(None, None, slot=slot)
    dev.set_tags(slot=slot), dev.set_sam_seq(False, slot=slot), dev.set_xa(0, slot=slot)


def test_text_plain(single):
    s = single
    got, base = _both(s, _plain)
    same_text(got, m.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"]))
    lines = got.splitlines()
    assert sum(1 for l in lines if int(l.split(b"\t")[1]) & 0x100 and b"S" in l.split(b"\t")[5]) > 100  # secondary lines are clipped
    assert all(l.split(b"\t")[9:11] == [b"*", b"*"] for l in lines if int(l.split(b"\t")[1]) & 0x100)  # ... and keep * *


def test_text_unmapped_mapq_hits_read_group(single):
    s = single

    def setup(dev, slot):
        _plain(dev, slot)
        dev.set_unmapped(True, slot=slot), dev.set_mapq(True, slot=slot), dev.set_tags(slot=slot, read_group="grp.1", hits=True)
    got, base = _both(s, setup)
    same_text(got, m.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"]))
    by_name = {l.split(b"\t", 1)[0]: l.split(b"\t") for l in got.splitlines() if int(l.split(b"\t")[1]) & 4}
    # a read the trims use up, and one of length 0: unmapped, the first with its whole read, the second with * *
    assert by_name[b"g11"][9] == s["reads"][11].upper() and by_name[b"g11"][10] == s["quals"][11].encode() and s["cl"][11] == (3, 3)
    assert by_name[b"g7"][9:11] == [b"*", b"*"]
    assert s["dev"].unmapped_count(slot=0) == s["dev"].unmapped_count(slot=1) > 0
    for slot in (0, 1):
        _plain(s["dev"], slot)


def test_text_sam_seq(single):
    s = single

    def setup(dev, slot):
        _plain(dev, slot)
        dev.set_sam_seq(True, slot=slot)
    got, base = _both(s, setup)
    same_text(got, m.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"], sam_seq=True))
    plain = _both(s, _plain)[0]
    assert got != plain and len(got) == len(plain)


def test_text_xa_with_a_budget_that_is_reached(single):
    s = single
    got_plain, base = _both(s, _plain)
    clipped = m.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"])
    want, n_entries = xa.apply(clipped, xa.ALL)
    assert xa.budget_stops(clipped) and n_entries > 1000  # the budget counts the entries with their clips
    s["dev"].set_xa(xa.ALL, slot=0)
    same_text(s["dev"].fetch_sam(slot=0)[0], want)
    assert s["dev"].xa_count(slot=0) == n_entries
    # the kept parts' own folding differs where the clips' bytes reach the budget first; the model on its folded text says the same
    s["dev"].set_xa(xa.ALL, slot=1)
    folded_base = s["dev"].fetch_sam(slot=1)[0]
    if s["dev"].xa_count(slot=1) == n_entries:
        same_text(m.apply(folded_base, s["reads"], s["quals"], s["cl"], s["rnames"]), want)
    for slot in (0, 1):
        _plain(s["dev"], slot)


def test_text_best_stratum_two_hits(single):
    s = single

    def setup(dev, slot):
        _plain(dev, slot)
        dev.set_report(0, 2, slot=slot)
    got, base = _both(s, setup)
    same_text(got, m.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"]))
    assert s["dev"].filtered_count(slot=0) == s["dev"].filtered_count(slot=1) > 0
    for slot in (0, 1):
        _plain(s["dev"], slot)


def test_bam_of_the_trimmed_text(single):
    s = single
    _plain(s["dev"], 0)
    s["dev"].set_unmapped(True, slot=0)
    text = bam_vs_sam(s["dev"], 0, [x.encode() for x in s["names"]], n_sam=1)  # levels 0 and 1 against the model's encoding of the text
    recs = [bm.decode(r, [x.encode() for x in s["names"]]) for r in bm.records(bm.sam_to_bam_payload(text, [x.encode() for x in s["names"]]))]
    assert len(recs) == len(text.splitlines())
    assert any(b"S" in l.split(b"\t")[5] for l in text.splitlines())
    _plain(s["dev"], 0)


# ---- 5. pairs ----

@functools.lru_cache(maxsize=None)
def _pair_case(orientation):
    """Pairs whose mates are 90 and 110 bases with tails of their own: the kept lengths differ mate by mate.  "rf": both mates
    reverse-complemented in front of their tails, the library whose mates point away from each other."""
    rng = np.random.default_rng(21)
    seqs, names = cases.reference(rng, False)
    n = 400
    r1, r2 = cases.make_rescue_pairs(rng, seqs, n, 90, 110, 2, 6, X, frac=0.3)
    reads, quals = [], []
    for r in r1 + r2:
        r = util.revcomp(r) if orientation == "rf" else r
        t = int(rng.integers(0, 25))
        reads.append(r + util.rand_seq(rng, t))
        quals.append("I" * len(r) + "#" * t)
    reads[4], quals[4] = reads[4][:20], quals[4][:20]  # a mate the fixed trims use up
    ref = fo.Reference(seqs)
    return dict(seqs=seqs, names=names, reads=reads, quals=quals, n=n, rnames=["p%d" % i for i in range(n)], e=2, ref=ref,
                idx=fo.OracleIndex(ref), trim=(12, 8, 20))


@pytest.mark.parametrize("orientation", ["fr", "rf"])
def test_pairs(orientation):
    c = _pair_case(orientation)
    kept_reads, kept_quals, cl = _kept(c)
    assert len(set(len(r) for r in kept_reads[:c["n"]])) > 5 and cl[4] == (12, 8)
    names2 = c["rnames"] + c["rnames"]
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        for slot in (0, 1):
            dev.set_pairs(I, X, slot=slot), dev.set_rescue(6, slot=slot), dev.set_rescue_discordant(True, slot=slot)
            dev.set_mapq(True, slot=slot), dev.set_unmapped(True, slot=slot), dev.set_orientation(orientation, slot=slot)
        _map(dev, c["reads"], names2, c["quals"], c["e"], c["trim"], slot=0)
        _map(dev, kept_reads, names2, kept_quals, c["e"], OFF, slot=1)
        got, base = dev.fetch_sam(slot=0)[0], dev.fetch_sam(slot=1)[0]
        clipped = m.apply(base, c["reads"], c["quals"], cl, c["rnames"], paired=True)
        same_text(got, clipped)
        counts = [(dev.pair_count(slot=k), dev.rescue_count(slot=k), dev.rescue_discordant_count(slot=k), dev.unmapped_count(slot=k)) for k in (0, 1)]
        assert counts[0] == counts[1] and min(counts[0][:2]) > 0 and counts[0][3] > 0, counts
        # the mate tags: MC is the other mate's clipped CIGAR, ms its whole qualities' score
        dev.set_mate_tags(True, slot=0)
        tagged = dev.fetch_sam(slot=0)[0]
        same_text(tagged, mt.apply(clipped, c["n"], c["quals"]))
        assert sum(1 for l in tagged.splitlines() if any(x.startswith(b"MC:Z:") and b"S" in x for x in l.split(b"\t")[11:])) > 100
        dev.set_mate_tags(True, slot=1)
        same_text(tagged, m.apply(dev.fetch_sam(slot=1)[0], c["reads"], c["quals"], cl, c["rnames"], paired=True))
        ref_names = [x.encode() for x in c["names"]]
        data = dev.fetch_bam(slot=0, level=1)[0]  # (MQ and ms have types of their own in BAM: the mate tags' model encodes them)
        assert b"".join(x[0] for x in bm.parse_bgzf(data, eof=False)) == mt.bam_payload(tagged, ref_names)
        dev.set_mate_tags(False, slot=0)
        assert bam_vs_sam(dev, 0, ref_names) == clipped
        a, b = dev.estimate_library(slot=0), dev.estimate_library(slot=1)
        assert a.orientation == b.orientation and [x.as_tuple() for x in a.by] == [x.as_tuple() for x in b.by]
        pa, pb = dev.fetch_pairs(slot=0), dev.fetch_pairs(slot=1)
        for f in ("rec_begin", "flag", "tid", "pos0", "nm", "cigar", "tlen"):
            assert np.array_equal(getattr(pa, f), getattr(pb, f)), f
    finally:
        dev.close()


# ---- 6. state ----

def test_refusals_slots_and_order():
    c = m.tails_case()
    kept_reads, kept_quals, cl = _kept(c)
    dev = open_device(c["seqs"], c["names"], c["idx"])[0]
    try:
        for bad in ((-1, 0, 0), (1025, 0, 0), (0, 1025, 0), (0, -1, 0), (0, 0, 94), (0, 0, -1)):
            dev.set_trim(1, 2, 3)
            with pytest.raises(FemError, match=r"^invalid argument: trim out of range"):
                dev.set_trim(*bad)
        # ... and left the setting as it was: (1, 2, 3) trims this batch
        batch = fo.ReadBatch(c["reads"])
        dev.stage_reads(batch.bases, batch.off)
        with pytest.raises(FemError, match=r"^call order violated: quality trimming"):  # the qualities are not committed
            dev.map_staged(e=c["e"])
        dev.stage_text(_q(c["quals"]), c["rnames"], quals_on_host=True)
        with pytest.raises(FemError, match=r"^call order violated: quality trimming"):  # ... or stayed on the host
            dev.map_staged(e=c["e"])
        dev.stage_text(_q(c["quals"]), c["rnames"])
        dev.map_staged(e=c["e"])
        assert [(int(a), int(b)) for a, b in zip(*dev.fetch_trim())] == m.batch_clips(c["quals"], 1, 2, 3)
        with pytest.raises(FemError, match=r"^call order violated: quality trimming"):
            dev.map_batch(batch.bases, batch.off, e=c["e"])  # fem_dev_map_batch_submit stages no qualities
        # fixed trims alone need no qualities before the mapping; a text with them kept on the host is refused
        dev.set_trim(5, 6, 0)
        dev.stage_reads(batch.bases, batch.off)
        dev.map_staged(e=c["e"])
        dev.stage_text(_q(c["quals"]), c["rnames"], quals_on_host=True)
        for fetch in (dev.fetch_sam, dev.fetch_bam):
            with pytest.raises(FemError, match=r"^invalid argument: a trimmed batch"):
                fetch()
        assert dev.trim_count() == (600, 600 * 11)
        # a packed batch
        from fem_amd import device
        hb, _ = dev.acquire_stage(600, 600 * 120)
        n_exc = device.pack_reads(batch.bases, 600, 120, hb)
        dev.commit_stage_packed(600, 120, n_exc)
        with pytest.raises(FemError, match=r"^input not supported by the device path: trimming"):
            dev.map_staged(e=c["e"])
        # two slots in flight with different settings; a set_trim between map and fetch acts on the next batch
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], (0, 0, 20), slot=0)
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], (7, 0, 0), slot=1)
        dev.set_trim(0, 0, 0, slot=0)
        dev.set_trim(0, 9, 0, slot=1)
        assert [(int(a), int(b)) for a, b in zip(*dev.fetch_trim(slot=1))] == [(7, 0)] * 600
        assert [(int(a), int(b)) for a, b in zip(*dev.fetch_trim(slot=0))] == cl
        text0 = dev.fetch_sam(slot=0)[0]
        assert len(m.clipped_reverse_lines(text0)) >= 100
        assert all(l.split(b"\t")[5].startswith(b"7S") or int(l.split(b"\t")[1]) & 16 for l in dev.fetch_sam(slot=1)[0].splitlines())
        # trimming off again: the bytes of a handle that never trimmed
        _map(dev, c["reads"], c["rnames"], c["quals"], c["e"], OFF, slot=0)
        off_again = dev.fetch_sam(slot=0)[0]
        with pytest.raises(FemError, match=r"^call order violated: the slot's batch was mapped without trimming"):
            dev.fetch_trim(slot=0)
        fresh = open_device(c["seqs"], c["names"], c["idx"])[0]
        try:
            batch = fo.ReadBatch(c["reads"])
            fresh.stage_reads(batch.bases, batch.off)
            assert fresh.stage_info()[1]  # packed, as ever
            fresh.stage_text(_q(c["quals"]), c["rnames"])
            fresh.map_staged(e=c["e"])
            assert fresh.fetch_sam()[0] == off_again
        finally:
            fresh.close()
        assert dev.stage_info(0)[1]  # the slot packs again once trimming is off
    finally:
        dev.close()


# ---- 7. FEM map --trim5 --trim3 --trim-qual ----

CLI_TRIM = (1, 2, 20)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A reference, its index, a FASTQ of single reads with tails and two of pairs, each beside its pre-trimmed twin."""
    from tests.harness import build_index
    tmp = tmp_path_factory.mktemp("trim")
    rng = np.random.default_rng(31)
    seqs, names = cases.reference(rng, False)
    fa = tmp / "ref.fa"
    fa.write_bytes(b"".join(b">%s desc\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    idx_path = str(tmp / "ref.idx")
    build_index(fa, idx_path)
    out = dict(tmp=tmp, fa=str(fa), idx=idx_path, names=names)

    def tailed(reads):
        full, quals = [], []
        for r in reads:
            t = int(rng.integers(0, 30))
            full.append(r + util.rand_seq(rng, t))
            quals.append("I" * len(r) + "#" * t)
        return full, quals

    def write(tag, reads, quals, rn):
        kr, kq, cl = m.kept(reads, quals, *CLI_TRIM)
        assert min(len(r) for r in kr) >= 35
        cases.write_fastq(tmp / (tag + ".fq"), reads, rn, quals, False)
        cases.write_fastq(tmp / (tag + "_kept.fq"), kr, rn, kq, False)
        return cl

    n = 1200
    s_reads, s_quals = tailed(util.make_reads(rng, seqs, n, 100, 2))
    s_reads[3] = s_reads[3].lower()
    out["single"] = dict(reads=s_reads, quals=s_quals, rnames=["s%d" % i for i in range(n)], cl=write("s", s_reads, s_quals, ["s%d" % i for i in range(n)]))
    n = 800
    r1, r2 = cases.make_rescue_pairs(rng, seqs, n, 90, 110, 2, 6, X, frac=0.3)
    (r1, q1), (r2, q2) = tailed(r1), tailed(r2)
    rn = ["m%d" % i for i in range(n)]
    out["pairs"] = dict(reads=r1 + r2, quals=q1 + q2, rnames=rn, cl=write("p1", r1, q1, rn) + write("p2", r2, q2, rn), n=n)
    return out


def _fem(files, out, reads, *args, bam=False):
    from tests.harness import counters, decode_bam_file, run_fem
    r = run_fem("map", "-e", "2", "-t", "16", "--ref", files["fa"], "--index", files["idx"], "-o", out, *reads, *args)
    assert r.returncode == 0, r.stderr.decode()
    got = decode_bam_file(out) if bam else open(out, "rb").read()
    return b"".join(l + b"\n" for l in got.splitlines() if not l.startswith(b"@")), counters(r.stderr), r.stderr.decode()


SWITCHES = ("--trim5", "1", "--trim3", "2", "--trim-qual", "20")


def _split(ctr):
    trim = [l for l in ctr if "trimmed" in l]
    return [l for l in ctr if "trimmed" not in l], trim


@pytest.mark.parametrize("batch", ["250", "100000"])
def test_cli_single_end(files, batch):
    s, tmp = files["single"], files["tmp"]
    opts = ("--batch", batch, "--unmapped", "--mapq")
    base, base_ctr, _ = _fem(files, str(tmp / "sk.sam"), ("--read1", str(tmp / "s_kept.fq")), *opts)
    got, ctr, _ = _fem(files, str(tmp / "s.sam"), ("--read1", str(tmp / "s.fq")), *opts, *SWITCHES)
    want = m.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"])
    same_text(got, want)
    rest, trim = _split(ctr)
    assert rest == base_ctr and not _split(base_ctr)[1]
    assert trim == ["The number of trimmed reads: %d" % m.counts(s["cl"])[0], "The number of trimmed bases: %d" % m.counts(s["cl"])[1]]
    assert len(m.clipped_reverse_lines(got)) >= 100
    if batch == "250":
        # two workers (here on one GPU): the batches are written as they retire, the lines and the summed counters are the same
        from tests.harness import counters, run_fem
        r = run_fem("map", "-e", "2", "-t", "16", "--ref", files["fa"], "--index", files["idx"], "-o", str(tmp / "s2.sam"), "--read1", str(tmp / "s.fq"),
                    *opts, *SWITCHES, "--gpus", "2", env=dict(FEM_TEST_SHARE_GPU="1", FEM_TESTING="1"))
        assert r.returncode == 0, r.stderr.decode()
        two = [l for l in open(str(tmp / "s2.sam"), "rb").read().splitlines() if not l.startswith(b"@")]
        assert sorted(two) == sorted(want.splitlines()) and counters(r.stderr) == ctr
        same_text(_fem(files, str(tmp / "s.bam"), ("--read1", str(tmp / "s.fq")), *opts, *SWITCHES, "--bam", bam=True)[0], want)
        turned = _fem(files, str(tmp / "st.sam"), ("--read1", str(tmp / "s.fq")), *opts, *SWITCHES, "--sam-seq", "-t", "24")[0]
        same_text(turned, m.apply(base, s["reads"], s["quals"], s["cl"], s["rnames"], sam_seq=True))


def test_cli_pairs(files):
    p, tmp = files["pairs"], files["tmp"]
    opts = ("--batch", "300", "--rescue", "6", "--mate-tags", "--unmapped")
    whole = ("--read1", str(tmp / "p1.fq"), "--read2", str(tmp / "p2.fq"))
    kept = ("--read1", str(tmp / "p1_kept.fq"), "--read2", str(tmp / "p2_kept.fq"))
    base, base_ctr, _ = _fem(files, str(tmp / "pk.sam"), kept, *opts)
    got, ctr, _ = _fem(files, str(tmp / "p.sam"), whole, *opts, *SWITCHES)
    want = m.apply(base, p["reads"], p["quals"], p["cl"], p["rnames"], paired=True)
    same_text(got, want)
    rest, trim = _split(ctr)
    assert rest == base_ctr
    assert trim == ["The number of trimmed reads: %d" % m.counts(p["cl"])[0], "The number of trimmed bases: %d" % m.counts(p["cl"])[1]]
    assert any(l.startswith("The number of rescued mates: ") and not l.endswith(": 0") for l in ctr)
    same_text(_fem(files, str(tmp / "p.bam"), whole, *opts, *SWITCHES, "--bam=0", bam=True)[0], want)
    # --infer-insert: the sample is trimmed as the run's reads are, so the learned range is the pre-trimmed run's
    got_i, _, err = _fem(files, str(tmp / "pi.sam"), whole, *opts, *SWITCHES, "--infer-insert=512")
    base_i, _, err_k = _fem(files, str(tmp / "pki.sam"), kept, *opts, "--infer-insert=512")
    line = [l for l in err.splitlines() if l.startswith("Inferred insert size range")]
    assert len(line) == 1 and line == [l for l in err_k.splitlines() if l.startswith("Inferred insert size range")]
    same_text(got_i, m.apply(base_i, p["reads"], p["quals"], p["cl"], p["rnames"], paired=True))
