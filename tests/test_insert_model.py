"""The insert size estimate's model (tests/insert_model.py: the rule of fem_dev_estimate_insert) on hand-built records."""
import pytest

from tests import insert_model as im
from tests import pair_model as pm

M100 = [(100, "M")]


def _rec(flag, tid, pos0, cigar=M100, nm=0):
    return (flag, tid, pos0, nm, cigar, "100")


def _fr(ins, start=1000, tid=0):
    """A pair whose mate 1 lies forward at `start` and whose mate 2 ends ins behind it, 100M each."""
    return [_rec(0, tid, start)], [_rec(16, tid, start + ins - 100)]


def _estimate(pairs):
    """pairs: (mate 1's records, mate 2's records) per pair."""
    res = pm.Records([a for a, _ in pairs] + [b for _, b in pairs])
    return im.estimate(res, len(pairs))


@pytest.mark.parametrize("n,ranks", [(1, (0, 0, 0)), (2, (0, 0, 0)), (4, (0, 1, 2)), (5, (1, 2, 3)), (64, (15, 31, 47)), (65, (16, 32, 48))])
def test_quantile_ranks(n, ranks):
    values = [200 + 7 * i for i in range(n)]
    order = [(37 * i + 11) % n for i in range(n)]  # (37 and n are coprime: a permutation)
    assert sorted(order) == list(range(n))
    e = _estimate([_fr(values[i]) for i in order])
    assert (e["q25"], e["q50"], e["q75"]) == tuple(values[r] for r in ranks)
    assert e["n_pairs"] == e["n_unique"] == e["n_informative"] == n


def test_equal_inserts_give_a_range_of_one_value():
    e = _estimate([_fr(300, start=1000 + i) for i in range(64)])
    assert im.as_tuple(e) == (64, 64, 64, 300, 300, 300, 300, 300, 1)


def test_the_lower_bound_stops_at_zero():
    # 32 pairs at 100 and 32 at 200: q25 = v[15] = 100, q75 = v[47] = 200, iqr = 100
    e = _estimate([_fr(100 if i < 32 else 200) for i in range(64)])
    assert (e["q25"], e["q50"], e["q75"]) == (100, 100, 200)
    assert (e["min_insert"], e["max_insert"], e["estimated"]) == (0, 500, 1)
    # and does not where it need not: 250 / 300, iqr = 50
    e = _estimate([_fr(250 if i < 32 else 300) for i in range(64)])
    assert (e["min_insert"], e["max_insert"]) == (100, 450)


def test_sixty_four_pairs_are_needed():
    pairs = [_fr(250 + i) for i in range(64)]
    e63, e64 = _estimate(pairs[:63]), _estimate(pairs)
    assert (e63["n_informative"], e63["estimated"], e63["min_insert"], e63["max_insert"]) == (63, 0, 0, 0)
    assert (e63["q25"], e63["q50"], e63["q75"]) == (265, 281, 296)  # the quartiles are there all the same
    assert (e64["n_informative"], e64["estimated"]) == (64, 1)
    assert (e64["min_insert"], e64["max_insert"]) == (265 - 3 * 32, 297 + 3 * 32)


def test_no_pair_at_all():
    assert im.as_tuple(_estimate([])) == (0, 0, 0, -1, -1, -1, 0, 0, 0)
    assert im.as_tuple(_estimate([([], [])] * 3)) == (3, 0, 0, -1, -1, -1, 0, 0, 0)


def test_the_largest_insert_counted():
    e = _estimate([_fr(im.INSERT_MAX), _fr(im.INSERT_MAX + 1)])
    assert (e["n_unique"], e["n_informative"], e["q25"], e["q75"]) == (2, 1, 16383, 16383)
    # the widest learned range still fits mate rescue's window
    wide = im.from_inserts(64, 64, [0] * 32 + [im.INSERT_MAX] * 32)
    assert (wide["min_insert"], wide["max_insert"]) == (0, 65532)


def test_a_deletion_in_the_reverse_mate_moves_the_insert():
    plain = _estimate([_fr(300)])
    a, _ = _fr(300)
    gapped = _estimate([(a, [_rec(16, 0, 1200, [(50, "M"), (2, "D"), (50, "M")], nm=2)])])
    inserted = _estimate([(a, [_rec(16, 0, 1200, [(50, "M"), (3, "I"), (47, "M")], nm=3)])])
    assert (plain["q50"], gapped["q50"], inserted["q50"]) == (300, 302, 297)
    # ... and one in the forward mate does not (its start counts, not its end)
    moved = _estimate([([_rec(0, 0, 1000, [(50, "M"), (2, "D"), (50, "M")], nm=2)], [_rec(16, 0, 1200)])])
    assert moved["q50"] == 300


@pytest.mark.parametrize("name,a,b,unique", [
    ("two records on one side", [_rec(0, 0, 1000), _rec(0, 0, 5000)], [_rec(16, 0, 1200)], 0),
    ("two records on the other", [_rec(0, 0, 1000)], [_rec(16, 0, 1200), _rec(16, 0, 1300)], 0),
    ("none on one side", [], [_rec(16, 0, 1200)], 0),
    ("none on the other", [_rec(0, 0, 1000)], [], 0),
    ("same strand, forward", [_rec(0, 0, 1000)], [_rec(0, 0, 1200)], 1),
    ("same strand, reverse", [_rec(16, 0, 1000)], [_rec(16, 0, 1200)], 1),
    ("other sequence", [_rec(0, 0, 1000)], [_rec(16, 1, 1200)], 1),
    ("forward mate behind the reverse one", [_rec(0, 0, 1201)], [_rec(16, 0, 1200)], 1),
    ("0x8000 on mate 1", [_rec(0x8000, 0, 1000, [])], [_rec(16, 0, 1200)], 0),
    ("0x8000 on mate 2", [_rec(0, 0, 1000)], [_rec(16 | 0x8000, 0, 1200, [])], 0),
])
def test_pairs_left_out(name, a, b, unique):
    e = _estimate([(a, b), _fr(300)])
    assert (e["n_pairs"], e["n_unique"], e["n_informative"], e["q50"]) == (2, unique + 1, 1, 300), name


def test_equal_starts_count():
    e = _estimate([([_rec(0, 0, 1000)], [_rec(16, 0, 1000)])])
    assert (e["n_informative"], e["q50"]) == (1, 100)


def test_mate_two_forward_counts():
    e = _estimate([([_rec(16, 0, 1250)], [_rec(0, 0, 1000)])])
    assert (e["n_unique"], e["n_informative"], e["q50"]) == (1, 1, 350)
