"""Reads too short to seed, in ragged batches, on every seeding front end — above all on the dense-index kernels
(seed_select_kernel + seed_join_kernel, whole and cut into banks), whose frequency loop once let a lane of a read of fewer than
k - 1 bases store behind its read's row: in the frequencies of the reads three or four places on and, from the later places of a
sub-block, in the next wave's read offsets and bases (fem_seed_select.hip.h, place_pack).  The other reads of such
a batch then lost candidates, differently on each run.

Every case is held to two arbiters: the oracle on the same batch (candidates, edit distances, end offsets, counters, records),
and, on the CPU, the oracle's own independence — the long reads of the batch have what they have without the short reads
beside them, and the short reads have nothing.  Each case is mapped twice on one slot and once on another: the three results
must be equal.  Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import cases
from tests import unmapped_model as um
from tests.harness import assert_same, assert_same_records, banked_device, build_index, counters, device_with_env, open_device, run_fem
from tests.harness import run_packed, same_text, stage_and_map

pytestmark = pytest.mark.gpu

FORMS = ("dense", "banked", "sparse", "hash")
KERNEL = {"dense": "seed_join_kernel", "banked": "seed_join_banked_kernel", "sparse": "seed_fast_kernel<lean>", "hash": "seed_fast_kernel<hash>"}
N_PLACED = 5 * 16 + 3  # five blocks of 16 reads and a short one
# placements at (e, longest read) = (3, 150): name -> (n, ((read, length), ..))
PLACEMENTS = {
    "first_and_last": (N_PLACED, ((0, 0), (N_PLACED - 1, 10))),
    "a_whole_block": (N_PLACED, tuple((32 + i, cases.short_lengths(3)[i % 7]) for i in range(16))),
    # neighbours inside a sub-block of five, across two sub-blocks, across two blocks, and at a block's first two places
    "neighbours": (N_PLACED, ((2, 0), (3, 10), (20, 10), (21, 0), (31, 5), (32, 0), (48, 0), (49, 0), (62, 72), (63, 10))),
    "only_the_last_is_long": (N_PLACED, tuple((i, cases.short_lengths(3)[i % 7]) for i in range(N_PLACED - 1))),
    "one_read": (1, ((0, 10),)),
    "seventeen": (17, ((0, 0),)),
}


def _placed(placement):
    n, short = PLACEMENTS[placement]
    return cases.short_reads_batch(1501 + n + len(short), 3, 150, n, short)  # (a seed at which the one long read of the fifth placement maps)


@pytest.fixture(scope="module")
def world():
    """One handle per front end over cases.short_reads_reference, opened when first asked for."""
    seqs, names, ref, idx = cases.short_reads_reference()
    devs = {}

    def device(form):
        if form not in devs:
            if form == "sparse":
                dev = open_device(seqs, names, idx)[0]
            else:
                dev = (banked_device(len(seqs[0]) + 2048 + 100) if form == "banked" else
                       device_with_env(**{"FEM_FORCE_DENSE" if form == "dense" else "FEM_FORCE_HASH": 1}))
                dev.upload_reference(seqs)
                dev.upload_reference_names(names)
                dev.upload_index(12, 3, idx.lookup, idx.occ[:idx.n_occ])
            if form in ("dense", "banked"):
                assert ("2 banks" in dev.index_info()) == (form == "banked"), dev.index_info()
            devs[form] = dev
        return devs[form]

    yield device
    for dev in devs.values():
        dev.close()


def _check_on_cpu(c):
    """The second arbiter, and that the case compares something: the oracle gives every long read what it gives it without the
    short reads, gives the short reads nothing, and maps half of the long reads or more."""
    n, short = len(c["reads"]), set(c["short"])
    got = cases.per_read(c["want"], n)
    assert all(got[r][0] == 0 and not any(got[r][1:]) for r in short)
    long_ids = [r for r in range(n) if r not in short]
    if long_ids:
        assert [got[r] for r in long_ids] == cases.per_read(c["want_long"], len(long_ids))
        assert int(c["want"].stats[1]) == int(c["want_long"].stats[1]) >= (len(long_ids) + 1) // 2, (c["want"].stats, len(long_ids))
        assert len(c["reads"][long_ids[0]]) == c["L"] == max(len(r) for r in c["reads"])
    else:
        assert int(c["want"].stats[1]) == 0


def _same_result(a, b):
    for x, y in zip(a.per_strand(), b.per_strand()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.stats, b.stats)


def _map_three_times(dev, c, form):
    """The batch on slot 0, again on slot 0, and on slot 1: each against the oracle, arrays and records."""
    batch = fo.ReadBatch(c["reads"])
    assert dev.seed_kernel(e=c["e"]) == KERNEL[form]
    results = []
    for slot in (0, 0, 1):
        got = dev.map_batch(batch.bases, batch.off, e=c["e"], slot=slot)
        results.append(got)
        assert_same(c["want"], got)
        assert_same_records(c["want"], dev.fetch_records(slot=slot))
    _same_result(results[0], results[1])
    _same_result(results[0], results[2])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("e,L", cases.SHORT_PARAMS)
def test_every_seventeenth_read_is_too_short(world, e, L, form):
    c = cases.short_reads_batch(170 + e + L, e, L)
    assert c["short"] == list(range(0, cases.SHORT_N, 17)) and sorted(set(r % 16 for r in c["short"])) == list(range(16))
    assert sorted(set(len(c["reads"][r]) for r in c["short"])) == sorted(cases.short_lengths(e))
    _check_on_cpu(c)
    _map_three_times(world(form), c, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("placement", sorted(PLACEMENTS))
def test_placements_of_the_short_reads(world, placement, form):
    c = _placed(placement)
    _check_on_cpu(c)
    _map_three_times(world(form), c, form)


@pytest.mark.parametrize("form", ["dense", "banked"])
def test_short_reads_print_as_unmapped_lines(world, form):
    e, L = 3, 150
    c = cases.short_reads_batch(170 + e + L, e, L)
    names = cases.short_reads_reference()[1]
    want = um.single_end(c["want"], names, c["reads"], c["rnames"], c["quals"])
    dev = world(form)
    dev.set_unmapped(True)
    try:
        stage_and_map(dev, c["reads"], c["rnames"], c["quals"], e)
        text, n_records, _, stats = dev.fetch_sam()
    finally:
        dev.set_unmapped(False)
    same_text(text, want)
    assert np.array_equal(stats, c["want"].stats)
    by_name = {l.split(b"\t", 1)[0]: l.split(b"\t") for l in text.splitlines() if int(l.split(b"\t")[1]) & 4}
    for r in c["short"]:
        f = by_name[c["rnames"][r].encode()]
        assert f[1:9] == [b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0"]
        assert f[9:11] == ([c["reads"][r], c["quals"][r].encode()] if c["reads"][r] else [b"*", b"*"])


@pytest.mark.parametrize("L", [5, 10, 11])
def test_a_packed_batch_of_short_reads_and_the_batch_behind_it(world, L):
    """Equal lengths go as 2-bit codes (the PACKED instance of seed_select_kernel): no read has a seed to select, nothing comes
    back; the next batch on the slot, an ordinary one, is the oracle's."""
    seqs, names, ref, idx = cases.short_reads_reference()
    dev = world("dense")
    rng = np.random.default_rng(40 + L)
    n = 83
    reads = [seqs[0][int(at):int(at) + L] for at in rng.integers(0, 190_000, n)]
    off, cand, ed, end, stats = run_packed(dev, reads, L, 3, 12, 3)
    want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=3)
    assert len(cand) == len(ed) == len(want.cands) == 0 and not np.any(off)
    assert np.array_equal(stats, want.stats) and int(stats[0]) == n and int(stats[1]) == 0
    c = _placed("first_and_last")
    batch = fo.ReadBatch(c["reads"])
    assert_same(c["want"], dev.map_batch(batch.bases, batch.off, e=3))
    assert_same_records(c["want"], dev.fetch_records())


# ---- FEM map on a dense index: reads that --trim5 uses up, reads that are all adapter ----

ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("short")
    seqs, names, ref, idx = cases.short_reads_reference()
    fa = tmp / "ref.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    build_index(fa, str(tmp / "ref.idx"))
    rng = np.random.default_rng(61)
    n = 600
    from tests import util
    reads = [util.make_reads(rng, seqs, 1, int(rng.integers(40, 151)), 2)[0] for _ in range(n)]
    rnames = ["c%d" % i for i in range(n)]
    assert 60 < sum(1 for r in reads if len(r) <= 60) < 200
    cases.write_fastq(tmp / "ragged.fq", reads, rnames, cases.quals(reads), False)
    planted = list(reads)
    for i in range(0, n, 17):  # all adapter (the adapter and what the sequencer reads behind it), or a base or ten in front of it
        k = (0, 1, 10)[(i // 17) % 3]
        planted[i] = (reads[i][:k] + ADAPTER + util.rand_seq(rng, 150))[:len(reads[i])]
    cases.write_fastq(tmp / "planted.fq", planted, rnames, cases.quals(planted), False)
    # reads that can map at e = 2 (37 + 12 e = 61 bases or more, src/filter.c:5-7): after --trim5 60, and beside the planted adapters
    can_map = {"ragged.fq": sum(1 for r in reads if len(r) >= 121), "planted.fq": sum(1 for i, r in enumerate(reads) if len(r) >= 61 and i % 17)}
    assert min(can_map.values()) >= 100
    return dict(tmp=tmp, fa=str(fa), idx=str(tmp / "ref.idx"), n=n, n_used_up=sum(1 for r in reads if len(r) <= 60), can_map=can_map)


def _fem_map(files, out, fq, env, *switches):
    r = run_fem("map", "-e", "2", "-t", "16", "--ref", files["fa"], "--index", files["idx"], "-o", out, "--read1", str(files["tmp"] / fq),
                "--batch", "250", "--unmapped", *switches, env=env)
    assert r.returncode == 0, r.stderr.decode()
    kernel = [l for l in r.stderr.decode().splitlines() if l.startswith("Seed kernel: ")]
    return open(out, "rb").read(), counters(r.stderr), kernel


@pytest.mark.parametrize("fq,switches", [("ragged.fq", ("--trim5", "60")), ("planted.fq", ("--adapter", ADAPTER.decode()))], ids=["trim5", "adapter"])
def test_cli_on_a_dense_index_equals_the_sparse_run(files, fq, switches):
    tmp = files["tmp"]
    sparse, sparse_ctr, sparse_kernel = _fem_map(files, str(tmp / "sparse.sam"), fq, None, *switches)
    dense, dense_ctr, dense_kernel = _fem_map(files, str(tmp / "dense.sam"), fq, dict(FEM_TESTING="1", FEM_FORCE_DENSE="1"), *switches)
    assert len(dense_kernel) == 1 and dense_kernel[0].startswith("Seed kernel: seed_join_kernel (index: dense"), dense_kernel
    assert len(sparse_kernel) == 1 and sparse_kernel[0].startswith("Seed kernel: seed_fast_kernel<lean> (index: sparse"), sparse_kernel
    same_text(dense, sparse)
    assert dense_ctr == sparse_ctr and dense_ctr
    lines = [l.split(b"\t") for l in dense.splitlines() if not l.startswith(b"@")]
    unmapped = sum(1 for f in lines if int(f[1]) & 4)
    mapped = len(set(f[0] for f in lines if not int(f[1]) & 4))
    assert unmapped + mapped == files["n"] and mapped >= files["can_map"][fq] // 2
    if fq == "ragged.fq":  # every read of 60 bases or less is used up: an unmapped line with its whole read
        assert unmapped >= files["n_used_up"]
    else:
        by_name = {f[0]: f for f in lines}
        assert all(int(by_name[b"c%d" % i][1]) & 4 for i in range(0, files["n"], 17))
