"""Mate rescue for pairs whose records do not pair (fem_dev_set_rescue_discordant: pair_probe_kernel and both search directions
in the rescue kernels, the rescued record in front of its mate's own lines in pair_kernel) against the plain-Python model of
tests/discordant_model.py on the oracle's single-end records.  Needs a GPU: -m gpu.

Every case first asserts on the model's result that its fixture does its job (tests/discordant_fixture.check_fixture).  Two
cases cannot reach the general figures (20 kept, 5 per mate): the 1000 bp case has 40 pairs in all and states its own, and
at E = e single-end mapping has already written nearly every hit the windows hold, so that case asks nothing of its fixture."""
import functools

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import bam_model as bm
from tests import discordant_fixture as df
from tests import discordant_model as dm
from tests import pair_model as pm
from tests import report_model as rp
from tests import rescue_model as rm
from tests import tags_model as tm
from tests import util
from tests.cases import write_fastq
from tests.harness import build_index, counters, fetch_sam, open_device, run_fem, same_pairs

pytestmark = pytest.mark.gpu

K_PAIR_ALONE = 32  # fem_tail.hip: pairs with more combinations are their wave's
I = 0


@functools.lru_cache(maxsize=None)
def case(seed, e, E, L, L2, n, X, repeats=False, near_end=False, lower=False, n_sym=6, copies=1, min_kept=20, min_each=5):
    """The batch, the oracle's single-end records and the model's result, checked: the fixture does its job."""
    rng = np.random.default_rng(seed)
    main = [util.rand_seq(rng, 60_000)]
    if repeats:
        main += util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200)
    seqs, r1, r2 = df.make_discordant_pairs(rng, main, n, L, L2, e, E, X, n_sym=n_sym, decoy_copies=copies, near_end=near_end)
    reads = r1 + r2
    if lower:  # a soft-masked reference and lower-case reads
        seqs = [s[:len(s) // 4] + s[len(s) // 4:3 * len(s) // 4].lower() + s[3 * len(s) // 4:] for s in seqs]
        reads = [r.lower() if i % 3 == 0 else r for i, r in enumerate(reads)]
    names = ["chr%d" % i for i in range(len(seqs))]
    rnames = ["p%d" % i for i in range(n)] * 2
    quals = ["".join(chr(33 + (11 * i + j) % 60) for j in range(len(r))) for i, r in enumerate(reads)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    want = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    ext, kept, traced, kinds = dm.rescue(want, n, reads, seqs, E, I, X)
    if E > e:
        df.check_fixture(kept, kinds, traced, n, min_kept, min_each)
    return dict(seqs=seqs, names=names, reads=reads, rnames=rnames, quals=quals, idx=idx, want=want, ext=ext, kept=kept,
                traced=traced, kinds=kinds, n=n, e=e, E=E, X=X)


def _device(c):
    return open_device(c["seqs"], c["names"], c["idx"])[0]


def _on(dev, c, slot, discordant=True):
    dev.set_pairs(I, c["X"], slot=slot)
    dev.set_rescue(c["E"], slot=slot)
    dev.set_rescue_discordant(discordant, slot=slot)


def _n_kind2(c):
    return sum(k == 2 for k, _ in c["kinds"].values())


def _check(dev, c, slot, qhost=False, packed=False):
    """The slot's text, counts and arrays equal the model's."""
    n, X = c["n"], c["X"]
    text, n_records, _, stats = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], slot, qhost, packed)
    assert np.array_equal(stats, c["want"].stats) and n_records == int(c["want"].rec_off[-1])  # single-end meaning kept
    assert text.decode("latin-1") == pm.sam_lines(c["ext"], n, c["names"], c["reads"], c["rnames"], c["quals"], I, X)
    _, n_proper = pm.expected(c["ext"], n, I, X)
    assert dev.pair_count(slot=slot) == n_proper and dev.rescue_count(slot=slot) == len(c["kept"])
    assert dev.rescue_discordant_count(slot=slot) == _n_kind2(c)
    same_pairs(dev.fetch_pairs(slot=slot), pm.pair_arrays(c["ext"], n, I, X))
    assert dev.rescue_count(slot=slot) == len(c["kept"]) and dev.rescue_discordant_count(slot=slot) == _n_kind2(c)
    return text


MAIN = (51, 2, 8, 100, 100, 400, 500)


def test_text_counts_and_arrays_equal_the_model():
    c = case(*MAIN)
    dev = _device(c)
    try:
        _on(dev, c, 1)
        dev.set_timing(True)
        dev.reset_timing()
        _check(dev, c, 1, packed=True)
        assert dev.kernel_time(10)[1] >= 1
        rec = dev.fetch_records(slot=1)  # single-end records untouched
        assert rec.n_records == int(c["want"].rec_off[-1])
        assert np.array_equal(rec.pos0, c["want"].r_pos) and np.array_equal(rec.nm, c["want"].r_nm)
    finally:
        dev.close()


def test_switch_off_again_is_rescue_alone():
    c = case(*MAIN)
    n, X = c["n"], c["X"]
    dev = _device(c)
    try:
        _on(dev, c, 1)
        on = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 1, packed=True)[0]
        dev.set_rescue_discordant(False, slot=1)
        off = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 1, packed=True)[0]
        assert dev.rescue_discordant_count(slot=1) == 0
        dev.set_pairs(I, X, slot=0)
        dev.set_rescue(c["E"], slot=0)  # a slot that only ever had set_rescue
        plain = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 0, packed=True)[0]
        ext1, kept1, _ = rm.rescue(c["want"], n, c["reads"], c["seqs"], c["E"], I, X)
        assert off == plain and on != off
        assert off.decode("latin-1") == pm.sam_lines(ext1, n, c["names"], c["reads"], c["rnames"], c["quals"], I, X)
        assert dev.rescue_count(slot=1) == len(kept1) == dev.rescue_count(slot=0)
        # the switch without rescue: a paired text, nothing rescued
        dev.set_rescue(None, slot=1)
        dev.set_rescue_discordant(True, slot=1)
        bare = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], c["e"], 1, packed=True)[0]
        assert bare.decode("latin-1") == pm.sam_lines(c["want"], n, c["names"], c["reads"], c["rnames"], c["quals"], I, X)
        assert dev.rescue_count(slot=1) == 0 and dev.rescue_discordant_count(slot=1) == 0
    finally:
        dev.close()


def test_switch_on_a_batch_without_discordant_pairs():
    c = case(*MAIN)
    n = c["n"]
    chosen = pm.choose(c["want"], n, I, c["X"])
    cnt = np.diff(c["want"].rec_off.astype(np.int64))
    keep = [i for i in range(n) if not (cnt[i] and cnt[n + i] and chosen[i] is None)]
    assert any(cnt[i] == 0 or cnt[n + i] == 0 for i in keep) and any(chosen[i] is not None for i in keep)
    sub = [c["reads"][i] for i in keep] + [c["reads"][n + i] for i in keep]
    sq = [c["quals"][i] for i in keep] + [c["quals"][n + i] for i in keep]
    sn = ["p%d" % i for i in keep] * 2
    dev = _device(c)
    try:
        _on(dev, c, 1)
        _on(dev, c, 0, discordant=False)
        t_on = fetch_sam(dev, sub, sn, sq, c["e"], 1)[0]
        t_off = fetch_sam(dev, sub, sn, sq, c["e"], 0)[0]
        assert t_on == t_off and dev.rescue_count(slot=1) == dev.rescue_count(slot=0) > 0
        assert dev.rescue_discordant_count(slot=1) == 0
    finally:
        dev.close()


def test_repeat_rich_reference_takes_the_probes_wave_path():
    c = case(61, 2, 8, 150, 100, 300, 500, repeats=True, copies=6)
    n, want = c["n"], c["want"]
    cnt = np.diff(want.rec_off.astype(np.int64))
    k2 = [r for r, (k, _) in c["kinds"].items() if k == 2]
    chosen = pm.choose(want, n, I, c["X"])
    disc = [i for i in range(n) if cnt[i] and cnt[n + i] and chosen[i] is None]
    assert any(cnt[i] * cnt[n + i] > K_PAIR_ALONE for i in disc)  # the probe's wave path
    big_kept = [r for r in k2 if cnt[r] * cnt[r - n if r >= n else r + n] > K_PAIR_ALONE]
    assert any(cnt[r - n if r >= n else r + n] > 1 for r in k2) and big_kept  # several anchors; a wave-path pair kept
    dev = _device(c)
    try:
        _on(dev, c, 0)
        _check(dev, c, 0)  # (mates of 150 and 100 bp: the reads go as characters)
    finally:
        dev.close()


# seed, e, E, L, L2, n, X, keywords of case(), quals on host, packed
VARIANTS = [
    (71, 3, 3, 100, 100, 300, 500, (), False, True),                                    # E = e
    (72, 2, 8, 100, 100, 300, 500, (("near_end", True),), True, True),                  # fragments at sequence ends, quals on host
    (73, 3, 8, 1000, 1000, 40, 3000, (("n_sym", 3), ("min_kept", 8), ("min_each", 2)), False, True),
    (74, 2, 8, 150, 150, 300, 600, (("lower", True),), False, False),                   # soft-masked reference, lower-case reads
]


@pytest.mark.parametrize("seed,e,E,L,L2,n,X,kw,qhost,packed", VARIANTS)
def test_variants_equal_the_model(seed, e, E, L, L2, n, X, kw, qhost, packed):
    c = case(seed, e, E, L, L2, n, X, **dict(kw))
    dev = _device(c)
    try:
        _on(dev, c, 0)
        _check(dev, c, 0, qhost, packed)
    finally:
        dev.close()


def test_with_mapq_unmapped_filter_and_tags():
    c = case(*MAIN)
    n, X, e = c["n"], c["X"], c["e"]
    want, dropped = rp.paired(c["want"], n, c["names"], c["reads"], c["rnames"], c["quals"], I, X, res=c["ext"],
                              rescued=set(c["kept"]), e=e, strata=1, max_hits=3)
    want = tm.apply(want, b"grp1", True)
    dev = _device(c)
    try:
        _on(dev, c, 0)
        dev.set_mapq(True)
        dev.set_unmapped(True)
        dev.set_report(strata=1, max_hits=3)
        dev.set_tags(read_group=b"grp1", hits=True)
        text = fetch_sam(dev, c["reads"], c["rnames"], c["quals"], e, 0, packed=True)[0]
        assert text.splitlines() == want.splitlines()
        assert dev.filtered_count() == dropped and dev.rescue_discordant_count() == _n_kind2(c)
        # a rescued mate with own records: its first line is the rescued record with MAPQ <= 40, its own lines follow with 0
        r = next(r for r, (k, _) in c["kinds"].items() if k == 2)
        data = dev.fetch_bam(level=0)
        payload = b"".join(m[0] for m in bm.parse_bgzf(data[0], eof=False))
        got = bm.bam_payload_to_sam(payload, [x.encode() for x in c["names"]])
        assert got.splitlines() == want.splitlines()
        mate = 0x80 if r >= n else 0x40
        mine = [l.split(b"\t") for l in want.splitlines() if l.split(b"\t")[0] == c["rnames"][r].encode() and int(l.split(b"\t")[1]) & mate]
        assert int(mine[0][1]) & 2 and not int(mine[0][1]) & 256 and int(mine[0][4]) <= 40
        assert all(int(f[1]) & 256 and int(f[4]) == 0 for f in mine[1:])
        # without the line filter NH and HI come from pair_kernel's own line index: the rescued record and the own ones are one slot
        dev.set_report()
        whole = tm.apply(rp.paired(c["want"], n, c["names"], c["reads"], c["rnames"], c["quals"], I, X, res=c["ext"],
                                   rescued=set(c["kept"]), e=e)[0], b"grp1", True)
        assert fetch_sam(dev, c["reads"], c["rnames"], c["quals"], e, 0, packed=True)[0].splitlines() == whole.splitlines()
        assert len(whole.splitlines()) == len(want.splitlines()) + dropped
        # one line per mate: of a rescued mate with own records the rescued record stays, the own ones go
        dev.set_report(strata=0, max_hits=1)
        one, gone = rp.paired(c["want"], n, c["names"], c["reads"], c["rnames"], c["quals"], I, X, res=c["ext"], rescued=set(c["kept"]),
                              e=e, strata=0, max_hits=1)
        assert gone >= _n_kind2(c)
        assert fetch_sam(dev, c["reads"], c["rnames"], c["quals"], e, 0, packed=True)[0].splitlines() == tm.apply(one, b"grp1", True).splitlines()
        assert dev.filtered_count() == gone
    finally:
        dev.close()


# ---- FEM map --rescue-discordant ----

def _map(fa, idx_path, p1, p2, out, *extra):
    return run_fem("map", "-e", "2", "-t", "4", "--ref", fa, "--index", idx_path, "--read1", p1, "--read2", p2, "-o", out, *extra,
                   text=True)


@pytest.mark.parametrize("gz", [False, True])
def test_cli_equals_the_model(tmp_path, gz):
    c = case(81 + gz, 2, 8, 100, 100, 1600, 500, min_kept=100)
    n, seqs = c["n"], c["seqs"]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">%s desc\n%s\n" % (nm.encode(), s) for nm, s in zip(c["names"], seqs)))
    idx_path = tmp_path / "ref.idx"
    build_index(fa, idx_path)
    r1, r2, q1, q2 = c["reads"][:n], c["reads"][n:], c["quals"][:n], c["quals"][n:]
    base = c["rnames"][:n]
    ext_ = ".fq.gz" if gz else ".fq"
    p1, p2 = tmp_path / ("r1" + ext_), tmp_path / ("r2" + ext_)
    write_fastq(p1, r1, [b + "/1" for b in base], q1, gz)
    write_fastq(p2, r2, [b + "/2" for b in base], q2, gz)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, len(s)) for nm, s in zip(c["names"], seqs))
    out = tmp_path / "out.sam"
    r = _map(fa, idx_path, p1, p2, out, "--batch", "700", "--rescue", "8", "--rescue-discordant")
    assert r.returncode == 0, r.stderr
    assert out.read_text(encoding="latin-1") == header + pm.sam_lines(c["ext"], n, c["names"], c["reads"], c["rnames"], c["quals"], I, 500)
    _, n_proper = pm.expected(c["ext"], n, I, 500)
    assert counters(r.stderr)[-3:] == ["The number of proper pairs: %d" % n_proper, "The number of rescued mates: %d" % len(c["kept"]),
                                        "The number of rescued discordant pairs: %d" % _n_kind2(c)]
    # without the flag: --rescue 8 alone, no such line
    ext1, kept1, _ = rm.rescue(c["want"], n, c["reads"], seqs, 8, I, 500)
    out1 = tmp_path / "out1.sam"
    r = _map(fa, idx_path, p1, p2, out1, "--batch", "700", "--rescue", "8")
    assert r.returncode == 0, r.stderr
    assert out1.read_text(encoding="latin-1") == header + pm.sam_lines(ext1, n, c["names"], c["reads"], c["rnames"], c["quals"], I, 500)
    assert "discordant" not in r.stderr and counters(r.stderr)[-1] == "The number of rescued mates: %d" % len(kept1)
