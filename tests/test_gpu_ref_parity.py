"""The kernels against what THE REFERENCE ITSELF computed: tests/golden/ref_*.npz hold small inputs and what a build of the
reference's own sources gave for them (tests/golden/make_ref_golden.py; tests/test_ref_parity.py holds the oracle against
the same files and, where oracle/_ref is built, against the live build).  Each fixture runs through

  * the sparse-index kernels (seed_fast_kernel) and the dense-index kernels (seed_select_kernel + seed_join_kernel,
    FEM_FORCE_DENSE under FEM_TESTING as smoke() does),
  * reads staged as characters and as 2-bit codes,
  * fem_dev_fetch (candidates, (ed, end), counters), fem_dev_fetch_records (the records' fields) and fem_dev_fetch_sam
    (the SAM text),

and through the command line (`FEM index` + `FEM map` on the fixture's files).  Everything is compared with the recorded
values of the reference, not with the oracle.  Needs a GPU: -m gpu."""
import os

import numpy as np
import pytest

from tests.golden import make_ref_golden as mg
from tests.harness import run_fem

pytestmark = pytest.mark.gpu

GOLDEN = os.path.dirname(os.path.abspath(mg.__file__))


def open_device(dense):
    from fem_amd import Device
    os.environ["FEM_FORCE_DENSE"] = "1" if dense else "0"
    try:
        return Device(0)
    finally:
        os.environ.pop("FEM_FORCE_DENSE")


def index_file_bytes(k, step, lookup, occ):
    """The file save_index writes (src/index.c:136-168): k, step, the lookup table, the occurrence count, the occurrences."""
    return (np.array([k, step], "<i4").tobytes() + np.ascontiguousarray(lookup, "<u4").tobytes() +
            np.array([len(occ)], "<u8").tobytes() + np.ascontiguousarray(occ, "<u8").tobytes())


class Recorded:
    """A fixture's records under the names oracle.fem_oracle.MapResult gives them (what tests.cases.expected_sam reads)."""

    def __init__(self, z):
        for key in mg.RECORD_KEYS:
            setattr(self, key, z[key])

    def cigar_str(self, j):
        return "".join("%d%s" % (int(o) >> 4, "MID"[int(o) & 0xF]) for o in self.cig[int(self.cig_off[j]):int(self.cig_off[j + 1])])

    def md_str(self, j):
        return self.md[int(self.md_off[j]):int(self.md_off[j + 1])].tobytes().decode()


def recorded_sam_body(inp, want):
    """The alignment lines of the reference's SAM file, rebuilt from the recorded fields; checked against the file's digest."""
    from tests.cases import expected_sam
    body = expected_sam(inp.names, inp.reads, inp.rnames, inp.quals, Recorded(want))
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(inp.names, inp.seqs))
    assert np.array_equal(mg.sha((header + body).encode()), want["sam_sha256"])
    return header, body


def stage(dev, inp, how, slot):
    """The case's reads into a slot: as characters (the copying entry point with packing switched off) or as 2-bit codes
    written by the caller (fem_dev_commit_stage_packed)."""
    from fem_amd import device
    from oracle import fem_oracle as fo
    batch = fo.ReadBatch(inp.reads)
    n, L = len(inp.reads), len(inp.reads[0])
    assert all(len(r) == L for r in inp.reads)
    if how == "chars":
        os.environ["FEM_NO_PACK"] = "1"
        try:
            dev.stage_reads(batch.bases, batch.off, slot=slot)
        finally:
            os.environ.pop("FEM_NO_PACK")
    else:
        hb, _ = dev.acquire_stage(n, n * L, slot=slot)
        dev.commit_stage_packed(n, L, device.pack_reads(batch.bases, n, L, hb), slot=slot)
    assert dev.stage_info(slot)[1] == (how == "packed")
    return batch


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("name", sorted(mg.CASES))
def test_kernels_reproduce_what_the_reference_computed(name, dense):
    case, want = mg.CASES[name], np.load(os.path.join(GOLDEN, name + ".npz"))
    inp = mg.stored_inputs(name)
    e, a = case["e"], case["a"]
    assert mg.defined_region(inp, e, a) and int((want["r_flag"] & 0x8000).sum()) == 0
    header, body = recorded_sam_body(inp, want)
    q = np.frombuffer("".join(inp.quals).encode(), np.uint8)
    dev = open_device(dense)
    try:
        dev.upload_reference(inp.seqs)
        dev.upload_reference_names(inp.names)
        n_occ, lookup, occ = dev.build_index(mg.K, mg.STEP)  # the index built on the device: the reference's file, byte for byte
        assert np.array_equal(mg.sha(index_file_bytes(mg.K, mg.STEP, lookup, occ[:n_occ])), want["index_sha256"])
        kernel = dev.seed_kernel(e=e, a=a)
        assert kernel == "seed_join_kernel" if dense else kernel.startswith("seed_fast_kernel"), kernel
        for slot, how in enumerate(("chars", "packed")):
            stage(dev, inp, how, slot)
            dev.stage_text(q, inp.rnames, slot=slot)
            dev.map_staged(e=e, a=a, slot=slot)
            got = dev.fetch(slot=slot)
            off, cand, ed, end = got.per_strand()
            assert np.array_equal(got.stats, want["stats"]), how
            assert np.array_equal(off, want["cand_off"]) and np.array_equal(cand, want["cands"]), how
            assert np.array_equal(ed, want["v_ed"]) and np.array_equal(end[ed != 0xFF], want["v_end"][want["v_ed"] != 0xFF]), how
            rec = dev.fetch_records(slot=slot)
            assert np.array_equal(rec.stats, want["stats"])
            for mine, theirs in (("rec_begin", "rec_off"), ("flag", "r_flag"), ("tid", "r_tid"), ("pos0", "r_pos"), ("nm", "r_nm"),
                                 ("cigar_off", "cig_off"), ("cigar", "cig"), ("md_off", "md_off"), ("md", "md")):
                assert np.array_equal(getattr(rec, mine), want[theirs]), (how, mine)
            text, n_records, n_asserted, stats = dev.fetch_sam(slot=slot)
            assert n_records == len(want["r_flag"]) and n_asserted == 0 and np.array_equal(stats, want["stats"])
            assert text.decode() == body, how  # QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL NM MD of every record
    finally:
        dev.close()


@pytest.mark.parametrize("key", sorted(mg.SWEEP))
def test_kernels_reproduce_the_recorded_sweep(key):
    # every e from 0 to 7 at its smallest defined read length and one above, a = 0, 1, 2, reads of 100 to 1 000 bases, two of
    # the reference's input batches: the counters, the records' fields and the SAM file against the digests recorded from
    # `FEM_ref map` (tests/golden/ref_recorded.npz; inputs from libfemhost's seeded generator)
    from oracle import fem_oracle as fo
    case = mg.SWEEP[key]
    e, a = case["e"], case["a"]
    z = np.load(mg.RECORDED)
    stats, want = z["sweep/%s/stats" % key], z["sweep/%s/digests" % key]
    inp = mg.sweep_inputs(case)
    assert mg.defined_region(inp, e, a)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(inp.names, inp.seqs))
    q = np.frombuffer("".join(inp.quals).encode(), np.uint8)
    batch = fo.ReadBatch(inp.reads)
    for dense in (False, True):
        dev = open_device(dense)
        try:
            dev.upload_reference(inp.seqs)
            dev.upload_reference_names(inp.names)
            n_occ, lookup, occ = dev.build_index(mg.K, mg.STEP)
            assert np.array_equal(mg.sha(index_file_bytes(mg.K, mg.STEP, lookup, occ[:n_occ])), want[0])
            dev.stage_reads(batch.bases, batch.off)
            dev.stage_text(q, inp.rnames)
            dev.map_staged(e=e, a=a)
            rec = dev.fetch_records()
            assert np.array_equal(rec.stats, stats), dense
            assert int(np.count_nonzero(rec.flag & 0x8000)) == 0
            got = dict(rec_off=rec.rec_begin.astype(np.uint64), r_flag=rec.flag, r_tid=rec.tid, r_pos=rec.pos0, r_nm=rec.nm,
                       r_mapq=np.full(rec.n_records, 255, np.uint8), cig_off=rec.cigar_off.astype(np.uint64), cig=rec.cigar,
                       md_off=rec.md_off.astype(np.uint64), md=rec.md)
            assert np.array_equal(mg.blob_sha(got, mg.RECORD_KEYS), want[2]), dense
            text, n_records, n_asserted, st = dev.fetch_sam()
            assert n_asserted == 0 and np.array_equal(st, stats)
            assert np.array_equal(mg.sha(header.encode() + text), want[1]), dense  # the SAM file of `FEM_ref map`, byte for byte
        finally:
            dev.close()


@pytest.mark.parametrize("name", sorted(mg.CASES))
def test_command_line_writes_the_references_files(tmp_path, name):
    case, want = mg.CASES[name], np.load(os.path.join(GOLDEN, name + ".npz"))
    inp = mg.stored_inputs(name)
    header, body = recorded_sam_body(inp, want)
    fa, fq = inp.write(str(tmp_path))
    ix, sam = str(tmp_path / "ref.idx"), str(tmp_path / "out.sam")
    r = run_fem("index", mg.K, mg.STEP, fa, ix)
    assert r.returncode == 0, r.stderr.decode()
    assert np.array_equal(mg.sha(open(ix, "rb").read()), want["index_sha256"])  # the SHA-256 of `FEM_ref index`'s file
    r = run_fem("map", "-e", case["e"], "-a", case["a"], "-t", "2", "--ref", fa, "--index", ix, "--read1", fq, "-o", sam)
    assert r.returncode == 0, r.stderr.decode()
    lines, theirs = open(sam).read().splitlines(), (header + body).splitlines()
    assert len(lines) == len(theirs)
    for mine, ref_line in zip(lines, theirs):  # field for field
        assert mine.split("\t") == ref_line.split("\t")
    err = r.stderr.decode()
    from oracle.ref_fem import COUNTER_LABELS
    for label, v in zip(COUNTER_LABELS, want["stats"]):
        assert "%s: %d\n" % (label, int(v)) in err


@pytest.mark.parametrize("e,a", [(0, 1), (3, 1), (7, 1), (3, 0), (2, 2)])
def test_one_seed_short_of_the_table_the_device_returns_no_candidates(e, a):
    # the reads of the second undefined region (tests/test_ref_parity.py): the reference reads uninitialised Seeds there, the
    # oracle returns no candidates, and so must both kernel families
    from oracle import fem_oracle as fo
    from tests import util
    rng = np.random.default_rng(950 + 10 * e + a)
    seqs = [util.rand_seq(rng, 20_000)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref, mg.K, mg.STEP)
    for dense in (False, True):
        dev = open_device(dense)
        try:
            dev.upload_reference(seqs)
            dev.upload_index(mg.K, mg.STEP, idx.lookup, idx.occ[:idx.n_occ])
            for L in range(mg.min_defined_length(e, a) - mg.STEP, mg.min_defined_length(e, a) + 1):
                batch = fo.ReadBatch(util.make_reads(rng, seqs, 64, L, 0))
                got = dev.map_batch(batch.bases, batch.off, e=e, a=a)
                want = fo.map_reads(ref, idx, batch, e=e, a=a)
                assert np.array_equal(got.stats, want.stats), (dense, L)
                if L < mg.min_defined_length(e, a):
                    assert got.n_candidates == 0 and int(got.stats[1]) == 0 and int(got.stats[3]) == 0, (dense, L)
                else:
                    assert int(got.stats[1]) >= 56 if e + 1 + a > 1 else int(got.stats[1]) == 0  # defined again: they map
        finally:
            dev.close()
