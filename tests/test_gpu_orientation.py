"""Library orientations on the device (fem_dev_set_orientation: the flips in pair_kernel, pair_probe_kernel, the rescue kernels
and insert_sample_kernel; fem_dev_estimate_library: library_sample_kernel) and FEM map --orientation, against the plain-Python
model of tests/orient_model.py on the oracle's single-end records of the same reads.  Needs a GPU: -m gpu.

Fixtures are made from FR fragments by the inverse of the model's reduction: FF is (mate 1, revcomp(mate 2)), RF is
(revcomp(mate 1), revcomp(mate 2)); the FR builders swap the mates half the time.  Reads are upper-case A C G T N."""
import functools
import re

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import bam_model as bm
from tests import discordant_fixture as df
from tests import insert_model as im
from tests import mate_tags_model as mt
from tests import orient_model as om
from tests import pair_model as pm
from tests import report_model as rp
from tests import tags_model as tm
from tests import util
from tests.cases import make_pairs, write_fastq
from tests.harness import build_index, counters, fetch_sam, open_device, run_fem, same_pairs

pytestmark = pytest.mark.gpu

K_PAIR_ALONE = 32  # fem_tail.hip: a pair with more combinations is its wave's
I, X = 0, 500


def oriented(r1, r2, orient):
    """An FR batch as a library of `orient` gives it."""
    return om.virtual_reads(list(r1) + list(r2), len(r1), orient)


def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _case(seqs, reads, e, n):
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    base = ["p%d_%s" % (i, "n" * (i % 7)) for i in range(n)]
    quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
    want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    return dict(seqs=seqs, names=["chr%d" % i for i in range(len(seqs))], reads=reads, rnames=base + base, quals=quals, idx=idx,
                want=want, n=n, e=e)


# ---- pairing ----

@functools.lru_cache(maxsize=None)
def pair_case(orient, repeats, L2=None):
    """600 pairs of `orient`: the two-sequence random reference (L = 100, e = 3), or the repeat-rich one of
    tests/test_gpu_pairs.py (64-base reads, e = 2).  On the latter one fragment in twelve comes from a repeat sequence, the
    others from the random one: adjacent copies of a unit let the records of an RF pair inside them pair as FR across two copies
    (the forward mate in the copy in front), so a batch drawn from the repeats alone has 125 FR proper pairs of 600 as an RF
    library and cannot show that FR is the wrong orientation for it; with one in twelve it is about 10, and some 20 pairs still
    have more than 32 combinations."""
    rng = np.random.default_rng(700 + 10 * orient + (5 if repeats else 0) + (L2 or 0))
    if repeats:
        seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200)
        seqs.append(util.rand_seq(rng, 120_000))
        L, e = 64, 2
    else:
        seqs = [util.rand_seq(rng, 200_000), util.rand_seq(rng, 50_000)]
        L, e = 100, 3
    n = 600
    r1, r2 = make_pairs(rng, [seqs[3]] * 11 + [seqs[1]] if repeats else seqs, n, L, e, L2)
    return _case(seqs, oriented(r1, r2, orient), e, n)


def _sam(dev, c, slot):
    return fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot)[0]


@pytest.mark.parametrize("orient,repeats,L2", [(om.RF, False, None), (om.FF, False, None), (om.RF, False, 75), (om.FF, False, 75),
                                               (om.RF, True, None), (om.FF, True, None)])
def test_paired_text_and_arrays_equal_the_model(orient, repeats, L2):
    c = pair_case(orient, repeats, L2)
    n, want = c["n"], c["want"]
    if repeats:  # the whole-wave path of pair_kernel
        cnt = np.diff(want.rec_off.astype(np.int64))
        assert int((cnt[:n] * cnt[n:] > K_PAIR_ALONE).sum()) >= 1
    lines, n_proper = om.expected(want, n, I, X, orient)
    assert n_proper > n // 5
    dev = _device(c)
    try:
        dev.set_pairs(I, X, slot=1)
        dev.set_orientation(om.NAMES[orient] if repeats else orient, slot=1)
        for mapq in (False, True):
            dev.set_mapq(mapq, slot=1)
            text = _sam(dev, c, 1)
            exp = om.paired_text(want, n, c["names"], c["reads"], c["rnames"], c["quals"], I, X, orient, e=c["e"] if mapq else None)
            assert text == exp
            assert dev.pair_count(slot=1) == n_proper
            same_pairs(dev.fetch_pairs(slot=1), om.pair_arrays(want, n, I, X, orient))
        dev.set_mapq(False, slot=1)
        text = _sam(dev, c, 1)
        assert [int(l.split(b"\t")[1]) for l in text.splitlines()] == [l[2] & 0x7FFF for l in lines]  # the rule, stated directly
        # the same batch as an FR library: next to no proper pairs, another text; a slot where the orientation was never set
        # and one where it was set to FR give the same bytes
        dev.set_pairs(I, X, slot=0)
        never = _sam(dev, c, 0)
        assert dev.pair_count(slot=0) < n // 20 and never != text
        assert never.decode("latin-1") == pm.sam_lines(want, n, c["names"], c["reads"], c["rnames"], c["quals"], I, X)
        dev.set_orientation(om.FR, slot=1)
        assert _sam(dev, c, 1) == never
        # the option survives set_pairs, as the other options do
        dev.set_orientation(orient, slot=1)
        dev.set_pairs(I, X, slot=1)
        assert _sam(dev, c, 1) == text
    finally:
        dev.close()


def test_set_orientation_refuses_other_values():
    from fem_amd import FemError
    c = pair_case(om.FF, False)
    dev = _device(c)
    try:
        for bad in (-1, 3, 16, "rr"):
            with pytest.raises(FemError):
                dev.set_orientation(bad)
    finally:
        dev.close()


# ---- rescue ----

E_RESCUE = 8


@functools.lru_cache(maxsize=None)
def rescue_case(orient):
    """tests/test_gpu_rescue_discordant.py's main fixture (pairs whose records do not pair, pairs with one heavy mate), as a
    library of `orient`."""
    rng = np.random.default_rng(51 + orient)
    n, L, e = 400, 100, 2
    seqs, r1, r2 = df.make_discordant_pairs(rng, [util.rand_seq(rng, 60_000)], n, L, L, e, E_RESCUE, X)
    return _case(seqs, oriented(r1, r2, orient), e, n)


def _kept_cover(c, kept, orient):
    """What a rescue test asks of its fixture, on the model alone: 20 kept records, both virtual strands of the anchor, both
    mates as the searched one."""
    assert len(kept) >= 20, len(kept)
    assert {bool(k["rc"]) for k in kept.values()} == {False, True}  # (B is searched reverse-complemented iff the anchor is virtually forward)
    assert {r >= c["n"] for r in kept} == {False, True}
    assert {k["real_flag"] for k in kept.values()} == {0, 16}


@pytest.mark.parametrize("orient", [om.RF, om.FF])
@pytest.mark.parametrize("discordant", [False, True])
def test_rescued_records_counts_and_text_equal_the_model(orient, discordant):
    c = rescue_case(orient)
    n, want = c["n"], c["want"]
    ext, kept, traced, kinds = om.rescued(want, n, c["reads"], c["seqs"], E_RESCUE, I, X, orient, discordant)
    _kept_cover(c, kept, orient)
    n_kind2 = sum(k == 2 for k, _ in kinds.values())
    assert (n_kind2 >= 10) == discordant
    dev = _device(c)
    try:
        dev.set_pairs(I, X, slot=1)
        dev.set_orientation(orient, slot=1)
        dev.set_rescue(E_RESCUE, slot=1)
        dev.set_rescue_discordant(discordant, slot=1)
        text = _sam(dev, c, 1)
        exp = om.paired_text(want, n, c["names"], c["reads"], c["rnames"], c["quals"], I, X, orient, ext=ext, rescued_reads=set(kept))
        assert text == exp
        _, n_proper = pm.expected(ext, n, I, X)
        assert dev.pair_count(slot=1) == n_proper and dev.rescue_count(slot=1) == len(kept)
        assert dev.rescue_discordant_count(slot=1) == n_kind2
        got = dev.fetch_pairs(slot=1)
        same_pairs(got, om.pair_arrays(want, n, I, X, orient, ext=ext))
        # the rescued records themselves: the lines of the kept reads that are no single-end record of theirs
        by_line = {}
        for k in range(len(got.flag)):
            by_line.setdefault((int(got.tid[k]), int(got.pos0[k]), int(got.flag[k]) & 16), []).append(k)
        for r, k in kept.items():
            tid, pos = k["record"][1], k["record"][2]
            assert (tid, pos, k["real_flag"]) in by_line, (r, k["record"])
    finally:
        dev.close()


# ---- the estimates ----

def _cut(seq, st, ins, L, orient, swap):
    a, b = seq[st:st + L], util.revcomp(seq[st + ins - L:st + ins])
    if swap:
        a, b = b, a
    return oriented([a], [b], orient)


@functools.lru_cache(maxsize=None)
def library_case(n_ff=300, n_fr=120, n_rf=80, n_eq=6):
    """Fragments of the three orientations in one batch, and a handful of pairs whose mates are cut from the same L bases."""
    rng = np.random.default_rng(733)
    L, e = 100, 3
    seqs = [util.rand_seq(rng, 200_000), util.rand_seq(rng, 50_000)]
    kinds = [om.FF] * n_ff + [om.FR] * n_fr + [om.RF] * n_rf + ["eq"] * n_eq
    r1, r2 = [], []
    for k, kind in enumerate(kinds):
        ins = L if kind == "eq" else int(np.clip(np.rint(rng.normal({om.FF: 300, om.FR: 220, om.RF: 400}[kind], 25)), 130, 600))
        a, b = _cut(seqs[k % 2], 500 + 90 * k, ins, L, om.FR if kind == "eq" else kind, bool(k & 1))
        r1.append(util.mutate(rng, a, int(rng.integers(0, 2)))[:L].ljust(L, b"A"))
        r2.append(b)
    order = rng.permutation(len(kinds))
    return _case(seqs, [r1[k] for k in order] + [r2[k] for k in order], e, len(kinds))


def _tuples(lib):
    return [e.as_tuple() for e in lib.by], lib.orientation


def _stage(dev, c, slot=0, text=True):
    batch = fo.ReadBatch(c["reads"])
    dev.stage_reads(batch.bases, batch.off, slot=slot)
    if text:
        dev.stage_text(np.frombuffer("".join(c["quals"]).encode("latin-1"), np.uint8), c["rnames"], slot=slot)
    dev.map_staged(e=c["e"], slot=slot)


def test_the_library_estimate_equals_the_model():
    c = library_case()
    n, want = c["n"], c["want"]
    model = om.library_estimate(want, n)
    counts = [e["n_informative"] for e in model["by"]]
    assert model["orientation"] == om.FF and counts[om.FF] > 250 and counts[om.FR] > 100 and counts[om.RF] > 60
    # the equal-pos0 pairs are informative under FR and under RF
    both = [i for i in range(n) if int(want.rec_off[i + 1]) - int(want.rec_off[i]) == 1 and int(want.rec_off[n + i + 1]) - int(want.rec_off[n + i]) == 1
            and om.insert_of(want, int(want.rec_off[i]), int(want.rec_off[n + i]), 0, im.INSERT_MAX, om.FR) is not None
            and om.insert_of(want, int(want.rec_off[i]), int(want.rec_off[n + i]), 0, im.INSERT_MAX, om.RF) is not None]
    assert len(both) >= 4
    assert len({tuple(sorted(e.items())) for e in model["by"]}) == 3  # three different estimates
    dev = _device(c)
    try:
        dev.set_pairs(0, 123)  # (the slot's own range plays no part)
        dev.set_orientation(om.RF)  # (nor does its orientation, in the library estimate)
        _stage(dev, c)
        plain = dev.fetch_sam()[0]
        _stage(dev, c)
        lib = dev.estimate_library()
        assert _tuples(lib) == ([im.as_tuple(e) for e in model["by"]], om.FF)
        assert dev.fetch_sam()[0] == plain  # the slot's options and the text that follows are untouched
        for o in (om.FR, om.RF, om.FF):
            dev.set_orientation(o)
            assert dev.estimate_insert().as_tuple() == lib.by[o].as_tuple()
    finally:
        dev.close()


def test_a_small_batch_gives_no_orientation():
    c = library_case(24, 10, 6, 0)
    assert c["n"] == 40
    model = om.library_estimate(c["want"], 40)
    assert model["orientation"] == -1 and sum(e["n_informative"] for e in model["by"]) >= 30
    dev = _device(c)
    try:
        from fem_amd import FemError
        with pytest.raises(FemError):
            dev.estimate_library()  # not in pair mode
        dev.set_pairs(0, 500)
        _stage(dev, c, text=False)
        assert _tuples(dev.estimate_library()) == ([im.as_tuple(e) for e in model["by"]], -1)
    finally:
        dev.close()


# ---- composition: every line option on an FF library ----

def test_ff_with_every_line_option():
    c = pair_case(om.FF, True)  # (the repeat-rich reference: mates with lines for the filter to drop)
    n, want = c["n"], c["want"]
    text = om.paired_text(want, n, c["names"], c["reads"], c["rnames"], c["quals"], I, X, om.FF, e=c["e"], unmapped=True)
    text, dropped = rp.apply(text, 1, None)
    exp = mt.apply(tm.apply(text, None, True), n, c["quals"])
    assert dropped > 0 and sum(int(l.split(b"\t")[1]) & 4 > 0 for l in exp.splitlines()) > 20
    dev = _device(c)
    try:
        dev.set_pairs(I, X)
        dev.set_orientation("ff")
        dev.set_unmapped(True)
        dev.set_mapq(True)
        dev.set_tags(hits=True)
        dev.set_mate_tags(True)
        dev.set_report(strata=1)
        got = _sam(dev, c, 0)
        assert got == exp
        assert dev.filtered_count() == dropped
        data = dev.fetch_bam(slot=0, level=0)
        payload = b"".join(m[0] for m in bm.parse_bgzf(data[0], eof=False))
        assert bm.bam_payload_to_sam(payload, [x.encode() for x in c["names"]]) == exp
    finally:
        dev.close()


# ---- FEM map --orientation ----

@functools.lru_cache(maxsize=None)
def cli_case():
    rng = np.random.default_rng(741)
    seqs = [util.rand_seq(rng, 150_000), util.rand_seq(rng, 60_000)]
    n = 600
    r1, r2 = make_pairs(rng, seqs, n, 100, 3)
    reads = oriented(r1, r2, om.FF)
    base = ["pair%d" % i for i in range(n)]
    quals = ["".join(chr(33 + (7 * i + j) % 40) for j in range(len(r))) for i, r in enumerate(reads)]
    ref = fo.Reference(seqs)
    want = fo.map_reads(ref, fo.OracleIndex(ref), fo.ReadBatch(reads), e=3, threads=4)
    return dict(seqs=seqs, n=n, reads=reads, base=base, quals=quals, want=want)


def _map(tmp_path, out, *extra):
    return run_fem("map", "-e", "3", "-t", "4", "--ref", tmp_path / "ref.fa", "--index", tmp_path / "ref.idx",
                   "--read1", tmp_path / "r1.fq", "--read2", tmp_path / "r2.fq", "-o", out, *extra, text=True)


def test_cli_orientation_ff_and_auto(tmp_path):
    c = cli_case()
    n, want = c["n"], c["want"]
    (tmp_path / "ref.fa").write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(c["seqs"])))
    build_index(tmp_path / "ref.fa", tmp_path / "ref.idx")
    write_fastq(tmp_path / "r1.fq", c["reads"][:n], [b + "/1" for b in c["base"]], c["quals"][:n], False)
    write_fastq(tmp_path / "r2.fq", c["reads"][n:], [b + "/2" for b in c["base"]], c["quals"][n:], False)
    header = "".join("@SQ\tSN:s%d\tLN:%d\n" % (i, len(s)) for i, s in enumerate(c["seqs"]))

    def model(lo, hi):
        text = om.paired_text(want, n, ["s0", "s1"], c["reads"], c["base"] * 2, c["quals"], lo, hi, om.FF)
        return header + text.decode("latin-1"), om.expected(want, n, lo, hi, om.FF)[1]

    # --orientation ff
    out = tmp_path / "ff.sam"
    r = _map(tmp_path, out, "--orientation", "ff")
    assert r.returncode == 0, r.stderr
    exp, n_proper = model(0, 500)
    assert out.read_text(encoding="latin-1") == exp and n_proper > n // 5
    assert counters(r.stderr)[-1] == "The number of proper pairs: %d" % n_proper
    assert "Inferred" not in r.stderr
    # --orientation auto --infer-insert=256: the orientation line names FF, the range line follows it
    auto = tmp_path / "auto.sam"
    r = _map(tmp_path, auto, "--orientation", "auto", "--infer-insert=256", "--batch", "100")
    assert r.returncode == 0, r.stderr
    sample = fo.map_reads(fo.Reference(c["seqs"]), fo.OracleIndex(fo.Reference(c["seqs"])),
                          fo.ReadBatch(c["reads"][:256] + c["reads"][n:n + 256]), e=3, threads=4)
    lib = om.library_estimate(sample, 256)
    assert lib["orientation"] == om.FF
    a, b, f = (e["n_informative"] for e in lib["by"])
    first = "Inferred library orientation: FF (FR %d, RF %d, FF %d informative of 256 pairs)." % (a, b, f)
    lines = r.stderr.splitlines()
    assert first in lines
    m = re.match(r"Inferred insert size range: (\d+)-(\d+) ", lines[lines.index(first) + 1])
    lo, hi = int(m.group(1)), int(m.group(2))
    assert (lo, hi) == (lib["by"][om.FF]["min_insert"], lib["by"][om.FF]["max_insert"])
    exp, n_proper = model(lo, hi)
    assert auto.read_text(encoding="latin-1") == exp
    assert counters(r.stderr)[-1] == "The number of proper pairs: %d" % n_proper
    # ... and the output is that of --orientation ff -I LO -X HI, whatever the batch size
    whole = tmp_path / "auto_whole.sam"
    r = _map(tmp_path, whole, "--orientation", "auto", "--infer-insert=256")
    assert r.returncode == 0, r.stderr
    given = tmp_path / "given.sam"
    r = _map(tmp_path, given, "--orientation", "ff", "-I", str(lo), "-X", str(hi), "--batch", "100")
    assert r.returncode == 0, r.stderr
    assert auto.read_bytes() == whole.read_bytes() == given.read_bytes()
