"""Every buffer of a handle is freed exactly once, and a buffer that regrows loses nothing: one slot takes a batch of read
pairs out every way the library has, then a batch of twice the reads while its buffers still hold the first one's sizes, with
fem_dbg_live_bytes (the counters kept by the one owning buffer type, fem_amd/csrc/fem_buf.hip.h) read before the handle is
opened, while it is open and after it is closed.  Once with default buffers, once with FEM_TEST_TINY_BUFFERS=1.
Needs a GPU: -m gpu."""
import os

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import bam_model as bm
from tests import pair_model as pm
from tests import rescue_model as rm
from tests import unmapped_model as um
from tests import util
from tests.cases import make_rescue_pairs
from tests.harness import assert_same, assert_same_records, check_members

pytestmark = pytest.mark.gpu

K, STEP, E, A = 12, 3, 3, 1
RESCUE_EDITS, I, X = 8, 0, 500
N_PAIRS, L = 512, 100


def _batch(rng, seqs, n):
    """n read pairs; a quarter with a mate of E + 1 .. RESCUE_EDITS edits (mate rescue finds it), some mates of random letters."""
    r1, r2 = make_rescue_pairs(rng, seqs, n, L, L, E, RESCUE_EDITS, X, frac=0.25)
    for i in range(n):
        u = rng.random()
        if u < 0.1:
            r1[i] = util.rand_seq(rng, L)
        elif u > 0.9:
            r2[i] = util.rand_seq(rng, L)
    return r1 + r2


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20261019)
    # three sequences of some 8 kbp, each a string of copies of four 300-base units between spacers
    seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=20, spacer=200)
    assert len(seqs) == 3 and sum(len(s) for s in seqs) <= 64_000
    w = dict(seqs=seqs, names=["chr%d" % i for i in range(3)], ref=fo.Reference(seqs))
    w["idx"] = fo.OracleIndex(w["ref"], K, STEP)
    for tag, n in (("first", N_PAIRS), ("second", 2 * N_PAIRS)):
        reads = _batch(rng, seqs, n)
        w[tag] = dict(n=n, reads=reads, batch=fo.ReadBatch(reads), want=fo.map_reads(w["ref"], w["idx"], fo.ReadBatch(reads), e=E, a=A, threads=8))
    f = w["first"]
    f["rnames"] = ["p%d_%s" % (i, "n" * (i % 40)) for i in range(N_PAIRS)] * 2
    f["quals"] = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(f["reads"])]
    f["withr"], f["kept"], _ = rm.rescue(f["want"], N_PAIRS, f["reads"], seqs, RESCUE_EDITS, I, X)
    assert len(f["kept"]) >= 10 and len(um.unmapped_reads(f["withr"], 2 * N_PAIRS)) >= 10
    f["sam"] = um.paired(f["want"], N_PAIRS, w["names"], f["reads"], f["rnames"], f["quals"], I, X, res=f["withr"], rescued=set(f["kept"]), e=E)
    return w


def _open(tiny):
    from fem_amd import Device
    assert os.environ.get("FEM_TESTING") == "1"
    os.environ["FEM_TEST_TINY_BUFFERS"] = "1" if tiny else "0"
    try:
        return Device(0)
    finally:
        os.environ.pop("FEM_TEST_TINY_BUFFERS")


def _map(dev, b, slot):
    dev.stage_reads(b["batch"].bases, b["batch"].off, slot=slot)
    dev.map_staged(e=E, a=A, k=K, step=STEP, slot=slot)


def _plain_and_packed(dev, b, slot):
    plain = dev.fetch(slot=slot)
    assert_same(b["want"], plain)
    packed = dev.fetch_packed(slot=slot)
    for x, y in zip(packed.per_strand(), plain.per_strand()):
        assert np.array_equal(x, y)
    assert np.array_equal(packed.stats, b["want"].stats) and packed.n_reads == 2 * b["n"]


@pytest.mark.parametrize("tiny", [False, True], ids=["default", "tiny-buffers"])
def test_every_buffer_is_freed_once_and_a_regrow_loses_nothing(world, tiny):
    from fem_amd.device import live_bytes
    w, f, slot = world, world["first"], 1
    base = live_bytes()  # (other modules may hold idle handles in this process)
    dev = _open(tiny)
    try:
        dev.upload_reference(w["seqs"])
        dev.upload_reference_names(w["names"])
        dev.upload_index(K, STEP, w["idx"].lookup, w["idx"].occ[:w["idx"].n_occ])
        n_occ, lookup, occ = dev.build_index(K, STEP)  # ... and the same index built on the device in its place
        assert n_occ == w["idx"].n_occ and np.array_equal(lookup, w["idx"].lookup) and np.array_equal(occ, w["idx"].occ[:n_occ])
        dev.set_pairs(I, X, slot=slot)
        dev.set_rescue(RESCUE_EDITS, slot=slot)
        dev.set_mapq(True, slot=slot)
        dev.set_unmapped(True, slot=slot)
        # the first batch, taken out every way
        q = np.frombuffer("".join(f["quals"]).encode("latin-1"), np.uint8)
        dev.stage_reads(f["batch"].bases, f["batch"].off, slot=slot)
        dev.stage_text(q, f["rnames"], slot=slot)
        dev.map_staged(e=E, a=A, k=K, step=STEP, slot=slot)
        _plain_and_packed(dev, f, slot)
        assert_same_records(f["want"], dev.fetch_records(slot=slot))
        text, n_records, _, stats = dev.fetch_sam(slot=slot)
        assert text == f["sam"] and n_records == int(f["want"].rec_off[-1]) and np.array_equal(stats, f["want"].stats)
        assert dev.rescue_count(slot=slot) == len(f["kept"])
        data, raw_len, n_blocks, n_rec_b, _, stats_b = dev.fetch_bam(slot=slot, level=1)
        payload = bm.sam_to_bam_payload(text, [x.encode() for x in w["names"]])
        assert raw_len == len(payload) and len(check_members(data, payload)) == n_blocks
        assert n_rec_b == n_records and np.array_equal(stats_b, stats)
        pairs = dev.fetch_pairs(slot=slot)
        for k, v in pm.pair_arrays(f["withr"], N_PAIRS, I, X).items():
            assert pairs.n_proper == v if k == "n_proper" else np.array_equal(getattr(pairs, k), v), k
        blob = bytes(np.random.default_rng(5).integers(65, 70, 100_000, dtype=np.uint8))
        check_members(dev.bgzf_compress(blob, 1), blob)
        held = live_bytes()
        assert held[0] > base[0] and held[1] > base[1]
        # twice the reads in the same slot: every per-batch buffer regrows while it holds the first batch's sizes
        _map(dev, w["second"], slot)
        _plain_and_packed(dev, w["second"], slot)
        grown = live_bytes()
        assert grown[0] > held[0] and grown[1] > held[1]
    finally:
        dev.close()
    assert live_bytes() == base
    # open, map, fetch, close once more in the same process
    dev = _open(tiny)
    try:
        dev.upload_reference(w["seqs"])
        dev.upload_index(K, STEP, w["idx"].lookup, w["idx"].occ[:w["idx"].n_occ])
        _map(dev, f, 0)
        assert_same(f["want"], dev.fetch(slot=0))
        assert live_bytes()[0] > base[0] and live_bytes()[1] > base[1]
    finally:
        dev.close()
    assert live_bytes() == base
