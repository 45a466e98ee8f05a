"""The rule of --rescue-discordant (include/fem_hip.h, fem_dev_set_rescue_discordant) as tests/discordant_model.py states it,
on hand-built records over small references, the searches and tracebacks through the oracle.  No GPU."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import discordant_fixture as df
from tests import discordant_model as dm
from tests import pair_model as pm
from tests import rescue_model as rm
from tests import util

M100 = [(100, "M")]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _seq(seed=1, n=8000):
    return bytearray(util.rand_seq(np.random.default_rng(seed), n))


def _copy(s, src, dst, k, L=100):
    """s[dst, dst + L) = s[src, src + L) with k substitutions."""
    c = bytearray(s[src:src + L])
    for u in range(k):
        x = 7 + 13 * u
        c[x] = ord("A") if c[x] != ord("A") else ord("C")
    s[dst:dst + L] = c


def _rec(flag, pos, nm=0):
    return (flag, 0, pos, nm, M100 if not flag & 0x8000 else [], "100" if not flag & 0x8000 else "")


def _run(s, m1, m2, read1, read2, E=4, I=0, X=500):
    res = pm.Records([m1, m2])
    return dm.rescue(res, 1, [read1, read2], [bytes(s)], E, I, X)


def test_a_pair_with_a_concordant_combination_is_no_candidate():
    s = _seq()
    # mate 2's second record pairs with mate 1's; mate 2 would also be found beside mate 1's other record
    _copy(s, 1300, 6300, 1)
    ext, kept, traced, kinds = _run(s, [_rec(0, 6000), _rec(0, 1000)], [_rec(0, 5000), _rec(16, 1300)], bytes(s[1000:1100]),
                                    util.revcomp(bytes(s[1300:1400])))
    assert not kept and not traced and not kinds and ext.rec_off.tolist() == [0, 2, 4]


def test_rescued_from_mate_1s_anchor():
    s = _seq(2)
    _copy(s, 5000, 1300, 3)  # mate 2 maps at 5000; beside mate 1 it lies 3 edits away
    ext, kept, traced, kinds = _run(s, [_rec(0, 1000)], [_rec(16, 5000)], bytes(s[1000:1100]), util.revcomp(bytes(s[5000:5100])))
    assert kinds == {1: (2, 0)} and kept[1]["record"][:4] == (16, 0, 1300, 3) and not traced[0]["tie"]
    assert ext.rec_off.tolist() == [0, 1, 3] and ext.r_pos.tolist() == [1000, 5000, 1300]  # behind B's own, which stays


def test_rescued_from_mate_2s_anchor():
    s = _seq(3)
    _copy(s, 6000, 2700, 2)  # mate 1 maps at 6000; beside mate 2 (reverse at 3000) it lies 2 edits away
    ext, kept, traced, kinds = _run(s, [_rec(0, 6000)], [_rec(16, 3000)], bytes(s[6000:6100]), util.revcomp(bytes(s[3000:3100])))
    assert kinds == {0: (2, 1)} and kept[0]["record"][:4] == (0, 0, 2700, 2)
    assert ext.rec_off.tolist() == [0, 2, 3] and ext.r_pos.tolist() == [6000, 2700, 3000]


def _both_directions(k0, k1, nm1=0, nm2=0):
    """Mate 1 exact at 1000 with mate 2's segment (k0 substitutions) beside it, mate 2 exact (reverse) at 5000 with mate 1's
    segment (k1 substitutions) beside it."""
    s = _seq(4)
    _copy(s, 5000, 1300, k0)
    _copy(s, 1000, 4700, k1)
    return _run(s, [_rec(0, 1000, nm1)], [_rec(16, 5000, nm2)], bytes(s[1000:1100]), util.revcomp(bytes(s[5000:5100])))


def test_equal_sums_in_both_directions_direction_0_wins():
    ext, kept, traced, kinds = _both_directions(2, 2)
    assert traced[0]["tie"] and kinds == {1: (2, 0)} and kept[1]["record"][:4] == (16, 0, 1300, 2)
    # the sum counts the anchor's NM: 1 + 2 against 0 + 3
    ext, kept, traced, kinds = _both_directions(2, 3, nm1=1, nm2=0)
    assert traced[0]["tie"] and kinds == {1: (2, 0)}


def test_direction_1_wins_with_the_smaller_sum():
    ext, kept, traced, kinds = _both_directions(3, 1)
    assert not traced[0]["tie"] and kinds == {0: (2, 1)} and kept[0]["record"][:4] == (0, 0, 4700, 1)
    assert ext.r_pos.tolist() == [1000, 4700, 5000]


def test_an_anchor_with_0x8000_is_skipped():
    s = _seq(5)
    _copy(s, 5000, 1300, 2)
    b = util.revcomp(bytes(s[5000:5100]))
    _, kept, traced, _ = _run(s, [_rec(0x8000, 1000), _rec(0, 6000)], [_rec(0, 7000)], bytes(s[1000:1100]), b)
    assert not kept and not traced
    _, kept, _, kinds = _run(s, [_rec(0, 1000), _rec(0, 6000)], [_rec(0, 7000)], bytes(s[1000:1100]), b)
    assert kinds == {1: (2, 0)} and kept[1]["a"] == 0


def test_the_ninth_record_is_no_anchor():
    s = _seq(6)
    _copy(s, 7000, 3200, 2)
    far = [_rec(0, 100 + 7 * i, 1) for i in range(8)]
    b = util.revcomp(bytes(s[7000:7100]))
    own = [_rec(0, 7000)]  # (as the record stands the strands agree: no combination pairs)
    _, kept, _, kinds = _run(s, far[:7] + [_rec(0, 3000)], own, bytes(s[3000:3100]), b)
    assert kinds == {1: (2, 0)} and kept[1]["a"] == 7
    _, kept, traced, _ = _run(s, far + [_rec(0, 3000)], own, bytes(s[3000:3100]), b)
    assert not kept and not traced


def test_a_hit_that_is_not_kept_leaves_the_pair_as_it_was():
    s = _seq(7)
    s[1499:1501] = b"CG"
    # direction 0: mate 2 (as searched) ends in an extra A.  The search ends it at 1499 (pos0 1400 = hi), sum 1; the traceback
    # folds the end insertion into the M run: 100M from 1401, an insert of 501 > X, not concordant with its anchor.
    # direction 1 has a hit with sum 2 that would be kept: it is not tried.
    read2 = util.revcomp(bytes(s[1401:1500]) + b"A")
    _copy(s, 1000, 4700, 2)
    m1, m2 = [_rec(0, 1000)], [_rec(16, 5000)]
    ext, kept, traced, kinds = _run(s, m1, m2, bytes(s[1000:1100]), read2)
    t = traced[0]
    assert not kept and not kinds and t["d"] == 0 and t["key"] == (1, 0, 0) and t["hit"][:2] == (1, 1400)
    assert t["start"] >= 0 and t["record"][2] == 1401 and not t["kept"]
    assert ext.rec_off.tolist() == [0, 1, 2] and ext.r_pos.tolist() == [1000, 5000]
    # with X = 501 that record is kept; and without direction 0's hit, direction 1's is
    _, kept, _, kinds = _run(s, m1, m2, bytes(s[1000:1100]), read2, X=501)
    assert kinds == {1: (2, 0)} and kept[1]["record"][2:4] == (1401, 1)
    _, kept, _, kinds = _run(s, m1, m2, bytes(s[1000:1100]), util.revcomp(bytes(s[5000:5100])))
    assert kinds == {0: (2, 1)} and kept[0]["record"][2:4] == (4700, 2)


def test_a_batch_of_kind_1_pairs_equals_rescue_model():
    rng = np.random.default_rng(11)
    seqs, r1, r2 = df.make_discordant_pairs(rng, [util.rand_seq(rng, 60_000)], 120, 100, 100, 2, 8, 500, n_sym=2)
    n = len(r1)
    ref = fo.Reference(seqs)
    want = fo.map_reads(ref, fo.OracleIndex(ref), fo.ReadBatch(r1 + r2), e=2, threads=4)
    _, _, _, kinds = dm.rescue(want, n, r1 + r2, seqs, 8, 0, 500)
    chosen = pm.choose(want, n, 0, 500)
    cnt = np.diff(want.rec_off.astype(np.int64))
    keep = [i for i in range(n) if not (cnt[i] and cnt[n + i] and chosen[i] is None)]
    assert 0 < len(keep) < n and sum(k == 2 for k, _ in kinds.values()) >= 10
    reads = [r1[i] for i in keep] + [r2[i] for i in keep]
    sub = fo.map_reads(ref, fo.OracleIndex(ref), fo.ReadBatch(reads), e=2, threads=4)
    ext, kept, traced, kinds = dm.rescue(sub, len(keep), reads, seqs, 8, 0, 500)
    ext0, kept0, traced0 = rm.rescue(sub, len(keep), reads, seqs, 8, 0, 500)
    assert len(kept) >= 10 and all(k == (1, 0 if r >= len(keep) else 1) for r, k in kinds.items())
    assert kept == kept0 and traced == traced0
    for f in ("rec_off", "r_flag", "r_tid", "r_pos", "r_nm", "cig_off", "cig", "md_off", "md"):
        assert np.array_equal(getattr(ext, f), getattr(ext0, f)), f


def test_output_lines_of_a_rescued_discordant_pair():
    s = _seq(8)
    _copy(s, 5000, 1300, 3)
    reads = [bytes(s[1000:1100]), util.revcomp(bytes(s[5000:5100]))]
    ext, kept, _, _ = _run(s, [_rec(0, 1000)], [_rec(16, 5000), _rec(0, 7000, 1)], reads[0], reads[1])
    assert list(kept) == [1]
    lines = pm.sam_lines(ext, 1, ["chr"], reads, ["p", "p"], ["I" * 100] * 2).splitlines()
    cols = [l.split("\t") for l in lines]
    # mate 1; then mate 2: the rescued record first (0x2, TLEN, no 0x100), its own records behind it in their order with 0x100
    assert [(int(c[1]), int(c[3]), c[6], int(c[7]), int(c[8])) for c in cols] == [
        (0x1 | 0x2 | 0x20 | 0x40, 1001, "=", 1301, 400),
        (0x1 | 0x2 | 0x10 | 0x80, 1301, "=", 1001, -400),
        (0x1 | 0x10 | 0x80 | 0x100, 5001, "=", 1001, 0),
        (0x1 | 0x80 | 0x100, 7001, "=", 1001, 0)]
    assert cols[1][9] != "*" and cols[2][9] == "*" and cols[3][9] == "*" and cols[1][11] == "NM:i:3"
    assert pm.expected(ext, 1)[1] == 1
