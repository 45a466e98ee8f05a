"""BAM output on the device: the BGZF compressor alone (fem_dev_bgzf_compress), fem_dev_fetch_bam against fem_dev_fetch_sam on
the same batches through the model of tests/bam_model.py, and FEM map --bam end to end.  Needs a GPU: -m gpu."""
import zlib

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import bam_model as bm
from tests import deflate_model as dm
from tests import util
from tests.cases import make_rescue_pairs, write_case, write_fastq
from tests.harness import bam_vs_sam, build_index, check_members, counters, decode_bam_file, open_device, open_sam_case, run_fem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from fem_amd import Device
    d = Device(0)
    yield d
    d.close()


def _compressor_inputs():
    rng = np.random.default_rng(5)
    period = util.rand_seq(rng, 32768)
    period2 = util.rand_seq(rng, 32769)
    return {
        "empty": b"", "one": b"x",
        "65279": bytes(rng.integers(0, 4, 65279, dtype=np.uint8) + 65),
        "65280": bytes(rng.integers(0, 4, 65280, dtype=np.uint8) + 65),
        "65281": bytes(rng.integers(0, 4, 65281, dtype=np.uint8) + 65),
        "zeros": bytes(200_000), "random": rng.bytes(150_000),
        "far32768": dm.far_match(32768), "far32767": dm.far_match(32767),
        # random letters with a period of 32768 and of 32769: three members each, cut off the period, that compress by their
        # 2-bit codes; of 64 three-letter words the latest occurrences are a few bytes back, so they say nothing of the window
        "dist32768": (period * 5)[:150_000], "dist32769": (period2 * 5)[:150_000],
        "runs258": b"".join(bytes([int(c)]) * int(n) for c, n in zip(rng.integers(0, 256, 2000), rng.integers(250, 600, 2000))),
        "illumina": bm.sam_to_bam_payload(bm.synthetic_sam(rng, 1500, 100, "illumina"), [b"chr1", b"chr2"]),
        "walk": bm.sam_to_bam_payload(bm.synthetic_sam(rng, 1500, 100, "walk"), [b"chr1", b"chr2"]),
    }


@pytest.mark.parametrize("level", [0, 1])
def test_compressor_alone(dev, level):
    for name, data in _compressor_inputs().items():
        out = dev.bgzf_compress(data, level)
        if not data:
            assert out == b""
            continue
        members = check_members(out, data)
        assert [len(m[0]) for m in members[:-1]] == [bm.MEMBER_INPUT] * (len(members) - 1), name
        if level == 0:
            assert all(m[2] == 0 for m in members), name
        elif name in ("zeros", "runs258", "dist32768", "illumina", "walk"):
            assert len(out) < len(data) // 2 if name != "walk" else len(out) < len(data), name
        if level == 1 and name in ("far32768", "far32767"):  # a 258-byte copy at the far end of the window is found
            assert (258, int(name[3:])) in dm.inflate(out, 18)[0][0].tokens, name


def test_compressor_ratio_against_zlib_level_1(dev):
    rng = np.random.default_rng(9)
    for profile in ("walk", "illumina"):
        payload = bm.sam_to_bam_payload(bm.synthetic_sam(rng, 4000, 100, profile), [b"chr1", b"chr2"])
        out = dev.bgzf_compress(payload, 1)
        members = check_members(out, payload)
        assert all(m[2] == 2 for m in members), profile  # dynamic Huffman blocks
        ref = 0
        for i in range(0, len(payload), bm.MEMBER_INPUT):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            ref += 26 + len(c.compress(payload[i:i + bm.MEMBER_INPUT]) + c.flush())
        print("%s: %.1f bytes per read, %.3f x zlib level 1" % (profile, len(out) / 4000, len(out) / ref))
        assert len(out) <= 1.08 * ref, (profile, len(out), ref)


@pytest.mark.parametrize("seed,e,L,n,repeats,odd", [(1, 3, 100, 1500, False, True), (2, 7, 150, 800, True, True),
                                                     (3, 2, 64, 3000, True, False), (4, 0, 36, 500, False, False),
                                                     (5, 7, 260, 700, False, True), (6, 4, 1024, 300, False, True)])
def test_fetch_bam_equals_fetch_sam(seed, e, L, n, repeats, odd):
    d, ref, idx, seqs, names, reads, rnames, quals = open_sam_case(seed, e, L, n, repeats, odd)
    try:
        batch = fo.ReadBatch(reads)
        q = np.frombuffer("".join(quals).encode(), np.uint8)
        d.stage_reads(batch.bases, batch.off, slot=1)
        d.stage_text(q, rnames, slot=1)
        d.map_staged(e=e, slot=1)
        text = bam_vs_sam(d, 1, [x.encode() for x in names], n_sam=True)
        assert text.count(b"\n") > min(n // 2, 60) or L < 40
        # the qualities on the host: no BAM
        d.stage_text(q, rnames, slot=1, quals_on_host=True)
        from fem_amd import FemError
        with pytest.raises(FemError, match="qualities"):
            d.fetch_bam(slot=1)
    finally:
        d.close()


def test_reads_without_records_and_name_limits():
    d, ref, idx, seqs, names, reads, rnames, quals = open_sam_case(11, 2, 100, 400, False, False)
    try:
        rng = np.random.default_rng(3)
        junk = [util.rand_seq(rng, 100) for _ in range(50)]  # (random reads: no records)
        reads2 = reads[:100] + junk
        batch = fo.ReadBatch(reads2)
        q = np.frombuffer(b"I" * len(batch.bases), np.uint8)
        for name_len, ok in ((254, True), (255, False)):
            rn = ["r%d" % i for i in range(len(reads2))]
            rn[0] = "n" * name_len
            d.stage_reads(batch.bases, batch.off, slot=0)
            d.stage_text(q, rn, slot=0)
            d.map_staged(e=2, slot=0)
            if ok:
                bam_vs_sam(d, 0, [x.encode() for x in names], n_sam=True)
            else:
                from fem_amd import FemError
                with pytest.raises(FemError, match="254"):
                    d.fetch_bam(slot=0)
        # no record at all
        nb = fo.ReadBatch(junk)
        d.stage_reads(nb.bases, nb.off, slot=0)
        d.stage_text(np.frombuffer(b"I" * len(nb.bases), np.uint8), ["j%d" % i for i in range(len(junk))], slot=0)
        d.map_staged(e=2, slot=0)
        data, raw_len, n_blocks, n_rec, _, _ = d.fetch_bam(slot=0)
        assert (data, raw_len, n_blocks, n_rec) == (b"", 0, 0, 0)
    finally:
        d.close()


@pytest.mark.parametrize("rescue", [None, 8])
def test_paired_fetch_bam_equals_fetch_sam(rescue):
    rng = np.random.default_rng(21)
    seqs = [util.rand_seq(rng, 200_000), util.rand_seq(rng, 60_000)]
    names = ["chr%d" % i for i in range(len(seqs))]
    d, ref, idx = open_device(seqs, names)
    try:
        n = 600
        r1, r2 = make_rescue_pairs(rng, seqs, n, 100, 120, 2, 8, 500)
        reads = r1 + r2
        batch = fo.ReadBatch(reads)
        q = np.frombuffer(b"".join(bytes(33 + (i + j) % 40 for j in range(len(r))) for i, r in enumerate(reads)), np.uint8)
        d.set_pairs(0, 500, slot=2)
        d.set_rescue(rescue, slot=2)
        d.stage_reads(batch.bases, batch.off, slot=2)
        d.stage_text(q, ["p%d" % (i % n) for i in range(2 * n)], slot=2)
        d.map_staged(e=2, slot=2)
        text = bam_vs_sam(d, 2, [x.encode() for x in names], n_sam=True)
        assert b"\t=\t" in text
        if rescue:
            assert d.rescue_count(slot=2) > 0
    finally:
        d.close()


# ---- FEM map --bam ----

def _map(*args):
    return run_fem("map", *args)


@pytest.mark.parametrize("gz", [False, True])
def test_cli_bam_single_end(tmp_path, gz):
    seqs, names, reads, rnames, quals, fa, fq = write_case(tmp_path, 91, 3, 100, 3000, gz)
    index_path = str(tmp_path / "ref.idx")
    build_index(fa, index_path)
    sam = str(tmp_path / "out.sam")
    r = _map("-e", "3", "-t", "3", "--ref", fa, "--index", index_path, "--read1", fq, "-o", sam, "--batch", "1000")
    assert r.returncode == 0, r.stderr.decode()
    want = open(sam, "rb").read()
    for flag in ("--bam", "--bam=0", "--bam=1"):
        out = str(tmp_path / "out.bam")
        rb = _map("-e", "3", "-t", "3", "--ref", fa, "--index", index_path, "--read1", fq, "-o", out, "--batch", "1000", flag)
        assert rb.returncode == 0, rb.stderr.decode()
        assert decode_bam_file(out) == want, flag
        assert counters(rb.stderr) == counters(r.stderr)
        data = open(out, "rb").read()
        assert data.endswith(bm.BGZF_EOF)
        if flag != "--bam=0":
            assert len(data) < len(want) // 2


def test_cli_bam_pairs_with_rescue(tmp_path):
    rng = np.random.default_rng(41)
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
    p1, p2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    write_fastq(p1, r1, [b + "/1" for b in base], q1, False)
    write_fastq(p2, r2, [b + "/2" for b in base], q2, False)
    common = ["-e", "2", "-t", "4", "--ref", str(fa), "--index", str(idx_path), "--read1", str(p1), "--read2", str(p2),
              "--batch", "700", "--rescue", "8"]
    sam = str(tmp_path / "out.sam")
    r = _map(*(common + ["-o", sam]))
    assert r.returncode == 0, r.stderr.decode()
    want = open(sam, "rb").read()
    for flag in ("--bam", "--bam=0"):
        out = str(tmp_path / "out.bam")
        rb = _map(*(common + ["-o", out, flag]))
        assert rb.returncode == 0, rb.stderr.decode()
        assert decode_bam_file(out) == want, flag
        assert counters(rb.stderr) == counters(r.stderr)
        assert any("rescued" in l for l in counters(rb.stderr))
