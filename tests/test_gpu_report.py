"""The line filter on the device (fem_dev_set_report: report_kernel and the kUnm instances of the text and BAM record kernels,
fem_tail.hip) against the plain-Python rule of tests/report_model.py, applied to the expected text of the other models on the
oracle's records and to the device's own unfiltered text.  Needs a GPU: -m gpu.  (The case generators below are also run
without one, by tests/test_report_model.py: they must give slots of every size at which the kernels take another path.)"""
import functools
import os
import subprocess

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import pair_model as pm
from tests import report_model as rp
from tests import rescue_model as rm
from tests import unmapped_model as um
from tests import util
from tests.test_gpu_bam import _bam_vs_sam, _decode_bam_file
from tests.test_gpu_pairs import _write_fastq, make_pairs
from tests.test_gpu_rescue import make_rescue_pairs
from tests.test_gpu_unmapped import _counter, _device, _map, _quals, _sam, _same, _stage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEM = os.path.join(ROOT, "fem_amd", "csrc", "FEM")
I, X = 0, 500

# (S, N); None: off
FILTERS = [(0, None), (None, 1), (1, 3), (None, 33), (2, 64), (15, 2 ** 31 - 1)]
# the slot sizes every case must hold: none, one, two, a lane's last (32), the wave's first (33), one step (64), two (65), many
SIZES = (0, 1, 2, 32, 33, 64, 65)
COPIES = (2, 32, 33, 64, 65, 210)


# ---- the cases ----

def _reference(rng, L, copies=COPIES):
    """Sequences: two repeat-rich ones (diverged copies: slots whose lines span several NM), a random one (one line), `exact`
    (for every k of `copies` a unit of its own in exactly k copies, each followed by a spacer of its own: k lines) and `loci`
    (one consensus unit at 12 loci, two clean and ten with 1 or 2 substitutions in the window [50, 50 + L), each followed by a
    flank of its own).  -> seqs, names, units [(unit, [offset of each copy in exact])], consensus, [(offset in loci, d)]."""
    rich = util.repeat_rich_reference(rng, n_seq=2, unit_len=300, n_units=4, copies=40, spacer=200)
    back = util.rand_seq(rng, 100_000)
    parts, n, units = [util.rand_seq(rng, 200)], 200, []
    for k in copies:
        u, at = util.rand_seq(rng, L + 60), []
        for _ in range(k):
            at.append(n)
            parts += [u, util.rand_seq(rng, L + 20)]
            n += 2 * L + 80
        units.append((u, at))
    cons = util.rand_seq(rng, 300)
    lparts, n, loci = [util.rand_seq(rng, 100)], 100, []
    for i in range(12):
        d = 0 if i < 2 else 1 + i % 2
        u = bytearray(cons)
        for pos in rng.choice(np.arange(60, 40 + L), d, replace=False):
            u[pos] = b"ACGT".replace(bytes([u[pos]]), b"")[int(rng.integers(0, 3))]
        loci.append((n, d))
        lparts += [bytes(u), util.rand_seq(rng, 300)]
        n += 600
    seqs = rich + [back, b"".join(parts), b"".join(lparts)]
    return seqs, ["chr%d" % i for i in range(len(seqs))], units, cons, loci


def _shuffled(rng, *lists):
    order = rng.permutation(len(lists[0]))
    return [[l[i] for i in order] for l in lists]


# seed, e, L, n
SINGLE_CASES = [(201, 3, 100, 1200), (202, 7, 150, 600)]


@functools.lru_cache(maxsize=None)
def single_case(seed, e, L, n):
    rng = np.random.default_rng(seed)
    seqs, names, units, cons, loci = _reference(rng, L)
    reads = util.make_reads(rng, seqs[:2], n // 2, L, min(e, 3), n_rate=0.002)
    reads += util.make_reads(rng, seqs[2:3], n // 4, L, e)
    for u, _ in units:  # 6 reads per unit, as they stand in it
        reads += [u[o:o + L] for o in rng.integers(0, 61, 6)]
    reads += [cons[50:50 + L]] * 6
    reads += [util.rand_seq(rng, L) for _ in range(n - len(reads))]
    reads, = _shuffled(rng, reads)
    rnames = ["read_%d_%s" % (i, "n" * (i % 20)) for i in range(n)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    return dict(seqs=seqs, names=names, reads=reads, rnames=rnames, quals=_quals(reads), e=e, ref=ref, idx=idx, res=res)


def _slot_nms(res, r):
    return res.r_nm[int(res.rec_off[r]):int(res.rec_off[r + 1])]


def check_slots(res, n_reads):
    """Slots of every size in SIZES and of 200 lines or more; 20 slots or more whose lines span three NM values or more."""
    counts = np.diff(res.rec_off.astype(np.int64))[:n_reads]
    for k in SIZES:
        assert np.count_nonzero(counts == k) >= 1, (k, sorted(set(counts.tolist())))
    assert np.count_nonzero(counts >= 200) >= 1, sorted(set(counts.tolist()))
    assert sum(1 for r in range(n_reads) if len(set(_slot_nms(res, r).tolist())) >= 3) >= 20


def check_single_case(c):
    check_slots(c["res"], len(c["reads"]))


# seed, e, L, n pairs, E of mate rescue (None: off)
PAIR_CASES = [(211, 3, 100, 700, None), (212, 2, 100, 700, 8)]


@functools.lru_cache(maxsize=None)
def pair_case(seed, e, L, n, E):
    rng = np.random.default_rng(seed)
    seqs, names, units, cons, loci = _reference(rng, L)
    exact, lseq = seqs[3], seqs[4]
    r1, r2 = [], []
    for u, at in units:  # mate 1 in the unit (all its copies), mate 2 in the spacer behind one copy (4 pairs) or nowhere near (2)
        for t in range(6):
            o = int(rng.integers(0, 61))
            sp = at[int(rng.integers(0, len(at)))] + len(u)
            r1.append(u[o:o + L])
            r2.append(util.revcomp(exact[sp + 5:sp + 5 + L]) if t < 4 else util.make_reads(rng, seqs[2:3], 1, L, 0)[0])
    for at, d in loci:  # mate 1 the consensus (NM 0 at the clean loci, d here), mate 2 in this locus' flank: chosen here
        if d:
            r1.append(cons[50:50 + L])
            r2.append(util.revcomp(lseq[at + 350:at + 350 + L]))
    k = n - len(r1)
    if E is None:
        a, b = make_pairs(rng, seqs[:3], k, L, e)
    else:  # a mate with e + 1 .. E edits in a quarter of the pairs: lost by the mapping, found by the rescue
        a, b = make_rescue_pairs(rng, seqs[:3], k, L, L, e, E, X, frac=0.25)
        for i in range(k):  # mates of random letters: lost for good
            if rng.random() < 0.1:
                a[i] = util.rand_seq(rng, L)
    r1, r2 = r1 + a, r2 + b
    for i in range(0, len(r1), 2):  # (the mates swapped in half the pairs)
        r1[i], r2[i] = r2[i], r1[i]
    r1, r2 = _shuffled(rng, r1, r2)
    reads = r1 + r2
    base = ["p%d_%s" % (i, "n" * (i % 30)) for i in range(n)]
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    res = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    withr, kept = None, {}
    if E is not None:
        withr, kept, _ = rm.rescue(res, n, reads, seqs, E, I, X)
    return dict(seqs=seqs, names=names, reads=reads, rnames=base + base, quals=_quals(reads), e=e, E=E, n=n, ref=ref, idx=idx,
                res=res, withr=withr, kept=kept)


def off_stratum_pairs(res, n_pairs):
    """Proper pairs in which a mate's chosen record has an NM above that mate's least."""
    found = 0
    for i, c in enumerate(pm.choose(res, n_pairs, I, X)):
        if c is not None:
            a, b = _slot_nms(res, i), _slot_nms(res, n_pairs + i)
            found += int(a[c[0]]) > int(a.min()) or int(b[c[1]]) > int(b.min())
    return found


def check_pair_case(c):
    after = c["withr"] if c["withr"] is not None else c["res"]
    check_slots(after, 2 * c["n"])
    assert off_stratum_pairs(after, c["n"]) >= 5
    if c["E"] is not None:
        assert len(c["kept"]) >= 20


# ---- expected texts (made once per case and switch) and the device ----

@functools.lru_cache(maxsize=None)
def _want_single(case, mapq):
    c = single_case(*case)
    return um.single_end(c["res"], c["names"], c["reads"], c["rnames"], c["quals"], e=c["e"] if mapq else None)


@functools.lru_cache(maxsize=None)
def _want_paired(case, mapq):
    c = pair_case(*case)
    return um.paired(c["res"], c["n"], c["names"], c["reads"], c["rnames"], c["quals"], I, X, res=c["withr"], rescued=set(c["kept"]),
                     e=c["e"] if mapq else None)


def _want(case, paired, mapq, unmapped):
    text = (_want_paired if paired else _want_single)(case, mapq)
    return text if unmapped else um.without_unmapped(text, paired)[0]


def _set(dev, slot, mapq, unmapped, strata, max_hits):
    dev.set_mapq(mapq, slot=slot)
    dev.set_unmapped(unmapped, slot=slot)
    dev.set_report(strata, max_hits, slot=slot)


def _check_filter(c, case, paired, strata, max_hits):
    n_lines_all = int((c["withr"] if paired and c["withr"] is not None else c["res"]).rec_off[-1])
    dev = _device(c)
    try:
        if paired:
            dev.set_pairs(I, X, slot=1)
            if c["E"] is not None:
                dev.set_rescue(c["E"], slot=1)
        ref_names = [x.encode() for x in c["names"]]
        for mapq in (False, True):
            for unmapped in (False, True):
                model = _want(case, paired, mapq, unmapped)
                want, dropped = rp.apply(model, strata, max_hits)
                _set(dev, 1, mapq, unmapped, None, None)
                plain = _sam(dev, c, 1)[0]
                _same(plain, model)
                assert dev.filtered_count(slot=1) == 0
                _set(dev, 1, mapq, unmapped, strata, max_hits)
                got, n_records, _, _ = _sam(dev, c, 1)
                _same(got, want)
                _same(got, rp.apply(plain, strata, max_hits)[0])
                if (strata, max_hits) == (15, 2 ** 31 - 1):
                    assert got == plain and dropped == 0
                else:
                    assert dropped > 0
                assert dev.filtered_count(slot=1) == dropped
                n_resc = dev.rescue_count(slot=1) if paired and c["E"] is not None else 0
                assert n_records == int(c["res"].rec_off[-1]) - dropped and n_records + n_resc == n_lines_all - dropped
                assert got.count(b"\n") == n_records + n_resc + dev.unmapped_count(slot=1)
                # BAM at both levels: the model's encoding of the device's own filtered text
                assert _bam_vs_sam(dev, 1, ref_names, n_sam=True) == got
                assert dev.filtered_count(slot=1) == dropped
                # the qualities on the host: qual_at still finds every primary line's field
                _same(_sam(dev, c, 1, quals_on_host=True)[0], want)
                assert dev.filtered_count(slot=1) == dropped
    finally:
        dev.close()


def _id(x):
    return "S%s_N%s" % tuple("off" if v is None else v for v in x)


@pytest.mark.parametrize("flt", FILTERS, ids=_id)
@pytest.mark.parametrize("case", SINGLE_CASES, ids=lambda x: "seed%d" % x[0])
def test_single_end_equals_the_model(case, flt):
    c = single_case(*case)
    check_single_case(c)
    _check_filter(c, case, False, *flt)


@pytest.mark.parametrize("flt", FILTERS, ids=_id)
@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda x: "seed%d" % x[0])
def test_pairs_equal_the_model(case, flt):
    c = pair_case(*case)
    check_pair_case(c)
    _check_filter(c, case, True, *flt)


def test_off_again_and_invalid_parameters():
    from fem_amd import FemError
    case = SINGLE_CASES[0]
    c = single_case(*case)
    dev = _device(c)
    try:
        off = _sam(dev, c, 0)[0]
        dev.set_report(0, 1, slot=1)
        got = _sam(dev, c, 1)[0]
        assert got == rp.apply(off, 0, 1)[0] and dev.filtered_count(slot=1) == off.count(b"\n") - got.count(b"\n") > 0
        dev.set_report(None, slot=1)
        assert _sam(dev, c, 1)[0] == off and dev.filtered_count(slot=1) == 0
        dev.set_report(max_hits=2, slot=1)
        assert _sam(dev, c, 1)[0] == rp.apply(off, None, 2)[0]
        for bad in (dict(strata=16), dict(strata=-2), dict(max_hits=0), dict(max_hits=-3), dict(max_hits=2 ** 31), dict(strata=0, max_hits=0)):
            with pytest.raises(FemError):
                dev.set_report(slot=1, **bad)
        assert _sam(dev, c, 1)[0] == rp.apply(off, None, 2)[0]  # (a refused call changes nothing)
        # the records and the pairs are not filtered
        _stage(dev, c, 1)
        assert dev.fetch_records(slot=1).n_records == int(c["res"].rec_off[-1])
    finally:
        dev.close()


def test_nothing_maps_and_an_empty_batch():
    rng = np.random.default_rng(220)
    c = dict(seqs=[util.rand_seq(rng, 5000)], names=["tiny"], e=3)
    c["reads"] = [util.rand_seq(rng, int(rng.integers(30, 160))) for _ in range(700)]
    c["rnames"] = ["x%d" % i for i in range(700)]
    c["quals"] = _quals(c["reads"])
    ref = fo.Reference(c["seqs"])
    c["idx"] = fo.OracleIndex(ref)
    res = fo.map_reads(ref, c["idx"], fo.ReadBatch(c["reads"]), e=3, threads=4)
    assert int(res.rec_off[-1]) == 0
    dev = _device(c)
    try:
        dev.set_report(0, 1)
        assert _sam(dev, c, 0)[:2] == (b"", 0) and dev.filtered_count() == 0
        dev.set_unmapped(True)
        text, n_records, _, _ = _sam(dev, c, 0)
        _same(text, um.single_end(res, c["names"], c["reads"], c["rnames"], c["quals"]))
        assert n_records == 0 and dev.unmapped_count() == 700 and dev.filtered_count() == 0
        _stage(dev, c, 0)
        _bam_vs_sam(dev, 0, [b"tiny"], n_sam=True)
        dev.set_pairs(I, X)
        _same(_sam(dev, c, 0)[0], um.paired(res, 350, c["names"], c["reads"], c["rnames"], c["quals"]))
        dev.set_unmapped(False)
        assert _sam(dev, c, 0)[0] == b""
        for unmapped in (False, True):
            dev.set_unmapped(unmapped)
            empty = dict(c, reads=[], rnames=[], quals=[])
            assert _sam(dev, empty, 0)[0] == b"" and dev.unmapped_count() == 0 and dev.filtered_count() == 0
    finally:
        dev.close()


def test_kernel_time_ids():
    rng = np.random.default_rng(9)
    c = dict(seqs=[util.rand_seq(rng, 100_000)], names=["c"], e=3)
    c["reads"] = util.make_reads(rng, c["seqs"], 300, 100, 3)[:280] + [util.rand_seq(rng, 100) for _ in range(20)]
    c["rnames"] = ["r%d" % i for i in range(300)]
    c["quals"] = ["I" * 100] * 300
    c["idx"] = fo.OracleIndex(fo.Reference(c["seqs"]))
    dev = _device(c)
    try:
        dev.set_timing(True)
        for flt, unmapped, pairs in ((None, False, False), ((0, None), False, False), ((None, 2), True, False), ((1, 2), True, True),
                                     (None, True, True), ((0, 1), False, True)):
            dev.set_report(*(flt or (None, None)))
            dev.set_unmapped(unmapped)
            dev.set_pairs(I, X) if pairs else dev.set_pairs(None)
            dev.reset_timing()
            for k in range(2):
                _stage(dev, c, 0)
                dev.fetch_sam()
                _stage(dev, c, 0)
                dev.fetch_bam(level=0)
            assert dev.kernel_time(15)[1] == (4 if flt else 0)
            assert dev.kernel_time(15)[0] > 0 or not flt
            assert dev.kernel_time(14)[1] == (4 if unmapped and not flt else 0)  # (the filter's line index is the unmapped reads' too)
            assert all(dev.kernel_time(i)[1] == 4 for i in (3, 4, 5))
            assert dev.kernel_time(7)[1] == 2 and dev.kernel_time(11)[1] == 2 and dev.kernel_time(13)[1] == 0
    finally:
        dev.close()


# ---- FEM map --strata / --max-hits ----

def test_cli(tmp_path):
    rng = np.random.default_rng(231)
    seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=4, copies=50, spacer=200) + [util.rand_seq(rng, 120_000)]
    names = ["s%d" % i for i in range(len(seqs))]
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">s%d desc\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    idx_path = str(tmp_path / "ref.idx")
    subprocess.run([FEM, "index", "12", "3", str(fa), idx_path], check=True, capture_output=True, timeout=600)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, len(s)) for nm, s in zip(names, seqs)).encode()
    n, e, E, S, N = 1500, 3, 8, 0, 2
    se = util.make_reads(rng, seqs, n, 100, e)
    x1, x2 = make_rescue_pairs(rng, seqs, n, 100, 100, e, E, X, frac=0.2)
    for i in range(n):
        u = rng.random()
        if u < 0.2:
            se[i] = util.rand_seq(rng, 100)
        if u < 0.1:
            x1[i] = util.rand_seq(rng, 100)
    q = ["".join(chr(33 + (7 * i + j) % 40) for j in range(100)) for i in range(n)]
    rn = ["r%d" % i for i in range(n)]
    files = {}
    for key, reads, suffix in (("se", se, ""), ("x1", x1, "/1"), ("x2", x2, "/2")):
        files[key] = tmp_path / (key + ".fq")
        _write_fastq(files[key], reads, [x + suffix for x in rn], q, False)
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    share = {"FEM_TESTING": "1", "FEM_TEST_SHARE_GPU": "1"}
    common = ["-e", str(e), "-t", "4", "--ref", str(fa), "--index", idx_path, "--batch", "400", "--gpus", "2", "--strata", str(S),
              "--max-hits", str(N)]
    # single-end
    res = fo.map_reads(ref, idx, fo.ReadBatch(se), e=e, threads=8)
    want, dropped = rp.single_end(res, names, se, rn, q, unmapped=False, strata=S, max_hits=N)
    assert dropped > n
    # read pairs with rescue, MAPQ and the unmapped reads' lines
    reads = x1 + x2
    resp = fo.map_reads(ref, idx, fo.ReadBatch(reads), e=e, threads=8)
    withr, kept, _ = rm.rescue(resp, n, reads, seqs, E, I, X)
    wantp, droppedp = rp.paired(resp, n, names, reads, rn + rn, q + q, I, X, res=withr, rescued=set(kept), e=e, strata=S, max_hits=N)
    assert len(kept) >= 20 and droppedp > n
    pargs = ["--read1", str(files["x1"]), "--read2", str(files["x2"]), "--rescue", str(E), "--mapq", "--unmapped"]
    for args, text, count in ((["--read1", str(files["se"])], want, dropped), (pargs, wantp, droppedp)):
        for bam in (False, True):
            out = str(tmp_path / "out")
            r = _map(*(common + args + ["-o", out] + (["--bam"] if bam else [])), env=share)
            assert r.returncode == 0, r.stderr.decode()
            got = _decode_bam_file(out) if bam else open(out, "rb").read()
            assert got.startswith(header)
            # (two workers: the batches' texts arrive in any order; a batch is whole reads / whole pairs)
            assert sorted(got[len(header):].splitlines()) == sorted(text.splitlines())
            assert rp.apply(got[len(header):], S, N) == (got[len(header):], 0)
            assert _counter(r.stderr, "filtered lines") == [count]
            err = r.stderr.decode().splitlines()
            k = next(i for i, l in enumerate(err) if l.startswith("The number of filtered lines"))
            assert err[k + 1].startswith("Time:")  # (behind the other counters)
    # without the switches: no such line on stderr
    r = _map("-e", str(e), "-t", "4", "--ref", str(fa), "--index", idx_path, "--read1", str(files["se"]), "-o", str(tmp_path / "off"))
    assert r.returncode == 0 and not _counter(r.stderr, "filtered lines")
