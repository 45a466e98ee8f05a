"""MC:Z, MQ:i and ms:i on the device (fem_dev_set_mate_tags: mate_score_kernel and the kMate instances of the text and BAM record
kernels, fem_tail.hip) and FEM map --mate-tags: the device's text and the decoded BAM records with the option on against the
plain-Python rule of tests/mate_tags_model.py applied to the same handle's output with the option off.  Needs a GPU: -m gpu.

Two cases of the issue's list cannot be built and are replaced by their nearest neighbours:
  * a mate CIGAR of exactly four operations: every CIGAR here begins and ends with M (the traceback takes an edit at a read's end
    as a mismatch), so the counts are odd; the indel case has 1, 3 (the writer's short path and its boundary), 5 (the first that
    takes the loop, as 4 would) and 9 to 15;
  * reads given without qualities: the C API has no such batch (fem_dev_commit_text_stage sends them, fem_dev_commit_names_stage
    keeps them on the host, which the option refuses); the tail's rule for it (no ms) is the model's test_no_qualities_no_ms."""
import functools
import re

import numpy as np
import pytest

from fem_amd.device import FemError
from oracle import fem_oracle as fo
from tests import bam_model as bm
from tests import mate_tags_model as mt
from tests import tags_model as tm
from tests import util
from tests.cases import I, LINE_E, LINE_RESCUE_E, MAX_HITS, RG, STRATA, X, line_options_case, make_pairs, write_fastq
from tests.harness import build_index, decode_bam_file, fetch_sam, open_device, pairing_on, run_fem, same_text

pytestmark = pytest.mark.gpu


def _rand_quals(rng, reads):
    """Qualities over the whole of '!'..'~': bytes on both sides of 48."""
    return [bytes(rng.integers(33, 127, len(r)).astype(np.uint8)).decode("latin-1") for r in reads]


def _case(seqs, r1, r2, e, rng, names=None):
    reads = r1 + r2
    base = ["m%d" % i for i in range(len(r1))]
    ref = fo.Reference(seqs)
    return dict(seqs=seqs, names=names or ["chr%d" % i for i in range(len(seqs))], reads=reads, rnames=base + base,
                quals=_rand_quals(rng, reads), e=e, n=len(r1), idx=fo.OracleIndex(ref), ref=ref)


def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _payload(dev, slot, level):
    data = dev.fetch_bam(slot=slot, level=level)
    return b"".join(m[0] for m in bm.parse_bgzf(data[0], eof=False)) if data[0] else b"", data[1]


def _check(dev, c, slot=0, level=0):
    """The slot's text and BAM records with mate tags == the model on the same handle's text without them -> (off, on)."""
    dev.set_mate_tags(False, slot=slot)
    off = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot)[0]
    assert mt.strip(off) == (off, [(None, None, None)] * off.count(b"\n"))
    bam_off = _payload(dev, slot, level)[0]
    dev.set_mate_tags(True, slot=slot)
    on = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot)[0]
    want = mt.apply(off, c["n"], c["quals"])
    same_text(on, want)
    assert mt.strip(on)[0] == off  # every byte in front of the tags is what it is without them
    names = [x.encode() for x in c["names"]]
    payload, raw_len = _payload(dev, slot, level)
    assert raw_len == len(payload)
    assert bm.bam_payload_to_sam(payload, names) == on  # block_size includes the tags: every record decodes to its line
    recs, recs_off = bm.records(payload), bm.records(bam_off)
    assert [mt.record_tags(r) for r in recs] == mt.strip(on)[1]  # MC:Z MQ:C ms:I, last and in this order
    for r, r_off, t in zip(recs, recs_off, mt.strip(on)[1]):  # ... behind the bytes the record has without them
        assert r[4:] == r_off[4:] + mt.aux(*t)
    return off, on


def _flags(line):
    return int(line.split(b"\t", 2)[1])


def _tag(line, tag):
    for f in line.rstrip(b"\n").split(b"\t")[11:]:
        if f.startswith(tag + b":"):
            return f[5:]
    return None


# ---- the repeat-rich case of tests/test_gpu_line_options.py (tests/cases.py): every option together ----

@pytest.mark.parametrize("variant", ["plain", "filter+rg+nh", "no mapq"])
def test_every_option_together(variant):
    c = dict(line_options_case(), e=LINE_E)
    dev = _device(c)
    try:
        pairing_on(dev, I, X, LINE_RESCUE_E)
        if variant == "filter+rg+nh":
            unfiltered = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], LINE_E, 0)[0]
            dev.set_report(strata=STRATA, max_hits=MAX_HITS)
            dev.set_tags(read_group=RG, hits=True)
        if variant == "no mapq":
            dev.set_mapq(False)
        off, on = _check(dev, c, level=1)
        assert dev.rescue_count() > 0 and dev.rescue_discordant_count() > 0  # a rescued mate is somebody's mate: its anchor's
        lines = on.splitlines()
        placed = [l for l in lines if _flags(l) & 4 and not _flags(l) & 8]
        assert placed and all(_tag(l, b"MC") and _tag(l, b"MQ") and _tag(l, b"ms") for l in placed)  # a placed unmapped line
        nothing = [l for l in lines if _flags(l) & 4 and _flags(l) & 8]
        assert nothing and all(_tag(l, b"ms") and not _tag(l, b"MC") and not _tag(l, b"MQ") for l in nothing)  # nothing maps: ms alone
        assert all(l.split(b"\t")[-1].startswith(b"ms:i:") for l in lines)  # the batch has qualities: ms on every line, last
        slots = [s for p in mt.pairs(on) for s in p if s]
        multi = [s for s in slots if len(s) > 1]
        assert multi and any(_tag(s[0], b"MC") for s in multi)  # secondary lines, tagged like their primary one
        assert all(len(set((_tag(l, b"MC"), _tag(l, b"MQ"), _tag(l, b"ms")) for l in s)) == 1 for s in multi)
        mqs = [int(_tag(l, b"MQ")) for l in lines if _tag(l, b"MQ")]
        if variant == "no mapq":
            assert mqs and set(mqs) == {255}
        else:
            assert 255 not in mqs and len(set(mqs)) > 1  # MQ follows the column
        if variant == "filter+rg+nh":
            assert dev.filtered_count() > 0
            # a slot that lost lines to the filter while its mate's tags still name its primary line
            full = {(s[0].split(b"\t", 1)[0], _flags(s[0]) & 0xC0): s for p in mt.pairs(unfiltered) for s in p if s}
            cut = [s for s in slots if len(full[(s[0].split(b"\t", 1)[0], _flags(s[0]) & 0xC0)]) > len(s)]
            assert cut
            by_key = {(s[0].split(b"\t", 1)[0], _flags(s[0]) & 0xC0): s for s in slots}
            seen = 0
            for s in cut:
                mate = by_key.get((s[0].split(b"\t", 1)[0], _flags(s[0]) & 0xC0 ^ 0xC0))
                if mate:
                    assert _tag(mate[0], b"MC") == s[0].split(b"\t")[5] and _tag(mate[0], b"MQ") == s[0].split(b"\t")[4]
                    seen += 1
            assert seen
            assert all(l.split(b"\t")[-4].startswith(b"RG:Z:") or not _tag(l, b"MC") for l in lines)  # behind RG
    finally:
        dev.close()


# ---- mate CIGARs of 1, 3, 5 and 9 to 15 operations: the writer's short path, its boundary and the loop ----

def _indel_read(frag, L, k):
    """frag's first bases with k edits, insertions and deletions in turn, evenly spaced."""
    out, prev = bytearray(), 0
    for j in range(k):
        cut = (j + 1) * L // (k + 1)
        out += frag[prev:cut]
        if j % 2 == 0:
            out.append([x for x in b"ACGT" if x != frag[cut] and x != frag[cut - 1]][0])
            prev = cut
        else:
            prev = cut + 1
    return bytes((out + frag[prev:])[:L])


@functools.lru_cache(maxsize=None)
def indel_case():
    rng, L = np.random.default_rng(905), 100
    seq = util.rand_seq(rng, 60_000)
    r1, r2 = [], []
    for i, k in enumerate([0, 1, 2, 4, 5, 6, 7, 1, 0, 4] * 2):  # mate 2 with k indels: beyond e, found by the rescue at E
        s0 = 1000 + 700 * i
        a, b = seq[s0:s0 + L], _indel_read(util.revcomp(seq[s0 + 150:s0 + 150 + L + 20]), L, k)
        if i % 4 == 3:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    return _case([seq], r1, r2, 2, rng)


def test_mate_cigars_short_path_boundary_and_loop():
    c = indel_case()
    dev = _device(c)
    try:
        dev.set_pairs(0, 500)
        dev.set_rescue(12)
        for unmapped in (False, True):
            dev.set_unmapped(unmapped)
            off, on = _check(dev, c)
            ops = sorted(set(len(re.findall(rb"\d+[MID]", _tag(l, b"MC"))) for l in on.splitlines() if _tag(l, b"MC")))
            assert ops[:3] == [1, 3, 5] and sum(k >= 8 for k in ops) >= 3, ops
            assert dev.rescue_count() >= 8
    finally:
        dev.close()


# ---- mates on different sequences; a mate whose primary line prints CIGAR * ----

def test_mates_on_different_sequences():
    rng, L = np.random.default_rng(906), 100
    seqs = [util.rand_seq(rng, 30_000), util.rand_seq(rng, 20_000), util.rand_seq(rng, 10_000)]
    r1 = [seqs[i % 3][500 + 90 * i:500 + 90 * i + L] for i in range(30)]
    r2 = [util.revcomp(seqs[(i + 1 + i % 2) % 3][700 + 80 * i:700 + 80 * i + L - i % 3]) for i in range(30)]
    c = _case(seqs, r1, r2, 2, rng, names=["first", "second_" + "n" * 70, "3"])
    dev = _device(c)
    try:
        dev.set_pairs(0, 500)
        dev.set_mapq(True)
        off, on = _check(dev, c)
        other = [l for l in on.splitlines() if l.split(b"\t")[6] not in (b"=", b"*")]
        assert len(other) >= 40 and all(_tag(l, b"MC") and _tag(l, b"MQ") and _tag(l, b"ms") for l in other)
    finally:
        dev.close()


def test_a_mate_whose_primary_line_prints_no_cigar():
    a = tm.asserted_case()
    rng = np.random.default_rng(907)
    n = len(a["reads"]) // 2
    c = dict(a, n=n, rnames=["a%d" % (i % n) for i in range(2 * n)], quals=_rand_quals(rng, a["reads"]))
    dev = _device(c)
    try:
        dev.set_pairs(0, 100_000)
        for mapq in (False, True):
            dev.set_mapq(mapq)
            off, on = _check(dev, c)
            seen = 0
            for pair in mt.pairs(on):
                for m in (0, 1):
                    if pair[m] and pair[m ^ 1] and pair[m][0].split(b"\t")[5] == b"*" and not _flags(pair[m][0]) & 4:
                        for l in pair[m ^ 1]:  # MQ and ms, no MC
                            assert _tag(l, b"MC") is None and _tag(l, b"MQ") == pair[m][0].split(b"\t")[4] and _tag(l, b"ms") is not None
                        seen += 1
            assert seen >= 1
    finally:
        dev.close()


# ---- mate_score_kernel: read lengths around its chunk, its group's span and a wave's; lines in two waves of sam_write_kernel ----

LENS = (1, 15, 16, 17, 63, 64, 65, 129, 300)


@functools.lru_cache(maxsize=None)
def lengths_case():
    """73 pairs: mate 1 of 99 to 111 bases, mate 2 of the lengths above.  Pair 0's mate 2 is too short to map and pairs 1 to 64
    have two lines each, so that without the lines of unmapped reads pair 32 has the lines 63 and 64 and pair 64 the lines 127 and
    128: one pair's slots in two waves of sam_write_kernel."""
    rng = np.random.default_rng(908)
    seq = util.rand_seq(rng, 120_000)
    l2 = [1] + [LENS[4 + i % 5] for i in range(64)] + [15, 16, 17, 1, 15, 16, 17, 16]
    r1, r2 = [], []
    for i, ln in enumerate(l2):
        s0 = 1000 + 900 * i
        r1.append(seq[s0:s0 + 99 + (5 * i) % 13])
        r2.append(util.revcomp(seq[s0 + 450 - ln:s0 + 450]))
    c = _case([seq], r1, r2, 2, rng)
    res = fo.map_reads(c["ref"], c["idx"], fo.ReadBatch(c["reads"]), e=2, threads=4)
    counts = np.diff(res.rec_off.astype(np.int64))
    assert all(int(k) == (1 if len(r) >= 63 else 0) for k, r in zip(counts, c["reads"])), counts
    starts = np.cumsum([0] + [len(r) for r in c["reads"]])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16))
    for ln in LENS:  # every length at a start that is no multiple of 16 (a batch's first read starts at 0)
        assert any(len(r) == ln and int(s) % 16 for r, s in zip(c["reads"], starts)), ln
    assert all(any(ord(ch) < 48 for ch in q) and any(ord(ch) >= 48 for ch in q) for q in c["quals"] if len(q) >= 63)
    return c


def test_scores_of_every_length_and_pairs_across_waves():
    c = lengths_case()
    n = c["n"]
    dev = _device(c)
    try:
        dev.set_pairs(0, 500)
        off, on = _check(dev, c)
        lines = on.splitlines()
        assert len(lines) > 128
        for k in (63, 127):  # one pair's two slots on both sides of a wave's last line
            assert lines[k].split(b"\t", 1)[0] == lines[k + 1].split(b"\t", 1)[0] and _flags(lines[k]) & 0x40 and _flags(lines[k + 1]) & 0x80
            assert _tag(lines[k], b"MC") == lines[k + 1].split(b"\t")[5] and _tag(lines[k + 1], b"MC") == lines[k].split(b"\t")[5]
        dev.set_unmapped(True)
        off, on = _check(dev, c)
        lines = on.splitlines()
        assert len(lines) == 2 * n
        # the scores against the plain sum: line 2i + m is mate m of pair i and carries the other mate's
        plain = [sum(ord(ch) - 33 for ch in q if ord(ch) - 33 >= 15) for q in c["quals"]]
        assert [int(_tag(l, b"ms")) for l in lines] == [plain[(1 - k % 2) * n + k // 2] for k in range(2 * n)]
        assert set(len(c["reads"][n + i]) for i in range(n)) == set(LENS)
    finally:
        dev.close()


# ---- on, off again, the kernel times, the refusal, a single-end slot ----

def test_on_then_off_again_is_a_fresh_handle_and_the_kernel_times():
    c = lengths_case()
    dev, fresh = _device(c), _device(c)
    try:
        for d in (dev, fresh):
            d.set_pairs(0, 500)
            d.set_unmapped(True)
            d.set_timing(True)
        run = lambda d: (fetch_sam(d, c["reads"], c["rnames"], c["quals"], c["e"], 0)[0], d.fetch_bam(level=0)[0])  # noqa: E731
        counts = lambda d: [d.kernel_time(k)[1] for k in range(17)]  # noqa: E731
        dev.set_mate_tags(True)
        dev.reset_timing()
        on = run(dev)
        on_counts = counts(dev)
        ms, launches = dev.kernel_time(17)
        assert launches == 2 and ms > 0.0  # one entry per fetch: the text's and the BAM's
        dev.set_mate_tags(False)
        dev.reset_timing()
        off = run(dev)
        assert dev.kernel_time(17) == (0.0, 0) and counts(dev) == on_counts  # ids 0-16 count as before
        fresh.reset_timing()
        plain = run(fresh)
        assert off == plain and on[0] != off[0] and on[1] != off[1]
        assert fresh.kernel_time(17) == (0.0, 0)
        assert on[0] == mt.apply(off[0], c["n"], c["quals"])
        # the qualities kept on the host with the option on: refused, text and BAM; off again: served
        dev.set_mate_tags(True)
        with pytest.raises(FemError, match=r"^invalid argument: mate tags \(fem_dev_set_mate_tags\)"):
            fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 0, quals_on_host=True)
        with pytest.raises(FemError, match=r"^invalid argument: mate tags \(fem_dev_set_mate_tags\)"):
            dev.fetch_bam()
        dev.set_mate_tags(False)
        assert fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 0, quals_on_host=True)[0] == off[0]
        # a single-end slot is unchanged by the setting, wherever its qualities are
        dev.set_pairs(None)
        fresh.set_pairs(None)
        single = fetch_sam(fresh, c["reads"], c["rnames"], c["quals"], c["e"], 0)[0]
        dev.set_mate_tags(True)
        dev.reset_timing()
        assert fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 0)[0] == single
        assert fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 0, quals_on_host=True)[0] == single
        assert dev.kernel_time(17) == (0.0, 0)
    finally:
        dev.close()
        fresh.close()


# ---- FEM map --read2 ... --mate-tags ----

def _in_batch_order(body):
    """The pairs of a text of several batches (which arrive in any order) in the order of their names m<i>."""
    pairs = sorted(mt.pairs(body), key=lambda p: int((p[0] or p[1])[0].split(b"\t", 1)[0][1:]))
    return b"".join(l for p in pairs for s in p if s for l in s)


def test_cli(tmp_path):
    rng = np.random.default_rng(909)
    seqs = util.repeat_rich_reference(rng, n_seq=2, unit_len=300, n_units=3, copies=12, spacer=200) + [util.rand_seq(rng, 60_000)]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = str(tmp_path / "ref.idx")
    build_index(fa, idx_path)
    n, e = 400, 2
    x1, x2 = make_pairs(rng, seqs, n, 100, e)
    for i in range(n):
        u = rng.random()
        if u < 0.1:
            x1[i] = util.rand_seq(rng, 100)
        if u < 0.04 or u > 0.9:
            x2[i] = util.rand_seq(rng, 100)
    q1 = ["".join(chr(33 + (7 * i + 3 * j) % 94) for j in range(100)) for i in range(n)]
    q2 = ["".join(chr(33 + (5 * i + 11 * j + 1) % 94) for j in range(100)) for i in range(n)]
    rn = ["m%d" % i for i in range(n)]
    p1, p2 = tmp_path / "x1.fq", tmp_path / "x2.fq"
    write_fastq(p1, x1, rn, q1, False)
    write_fastq(p2, x2, rn, q2, False)
    out = str(tmp_path / "out")
    common = ["-e", str(e), "-t", "4", "--ref", str(fa), "--index", idx_path, "--read1", str(p1), "--read2", str(p2), "--unmapped", "--mapq",
              "--rescue", "8", "--nh", "-o", out]

    def body(*args, bam=False, env=None):
        r = run_fem("map", *(common + list(args)), env=env)
        assert r.returncode == 0, r.stderr.decode()
        got = decode_bam_file(out) if bam else open(out, "rb").read()
        return _in_batch_order(b"".join(l + b"\n" for l in got.splitlines() if not l.startswith(b"@")))

    plain = body("--batch", "150")
    assert plain.count(b"\n") >= 2 * n and mt.strip(plain)[0] == plain and b"\tms:i:" not in plain
    want = mt.apply(plain, n, q1 + q2)
    shapes = [l for l in want.splitlines()]
    assert any(_flags(l) & 4 and _tag(l, b"MC") for l in shapes) and any(_flags(l) & 4 and not _tag(l, b"MQ") for l in shapes)
    assert any(_flags(l) & 0x100 and _tag(l, b"MC") for l in shapes)
    same_text(body("--batch", "150", "--mate-tags"), want)
    same_text(body("--batch", "64", "--mate-tags"), want)  # small batches: the same bytes
    same_text(body("--batch", "7", "--mate-tags", "--gpus", "1"), want)
    same_text(body("--batch", "150", "--mate-tags", "--bam", bam=True), want)
    assert body("--batch", "150", "--bam", bam=True) == plain
    # with the read group's tag, the line filter, discordant rescue and a learned insert range, on two workers
    more = ["--batch", "150", "--rg", "@RG\\tID:lane.1", "--strata", "1", "--rescue-discordant", "--infer-insert=256"]
    plain2 = body(*more)
    assert plain2 != plain and b"\tRG:Z:lane.1\n" in plain2
    share = {"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"}  # (--gpus 2: two workers on the one GPU)
    same_text(body(*(more + ["--mate-tags", "--gpus", "2"]), env=share), mt.apply(plain2, n, q1 + q2))
