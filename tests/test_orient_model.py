"""tests/orient_model.py against itself: the rule stated directly and its reduction to the FR models choose the same combinations
and give the same lines on random hand-built records, FR is pair_model exactly, and the library estimate's choice is pinned.
No GPU."""
import numpy as np
import pytest

from tests import insert_model as im
from tests import orient_model as om
from tests import pair_model as pm


def _random_batch(rng, n_pairs):
    """Hand-built records: three sequences, both strands, a few 0x8000 records, many equal pos0, indel CIGARs, 0-5 records per
    read, positions close enough that a good share of the combinations is concordant under some orientation."""
    per_read = []
    centres = rng.integers(100, 2000, n_pairs)
    for k in range(2 * n_pairs):
        c = int(centres[k % n_pairs])
        recs = []
        for t in range(int(rng.integers(0, 6))):
            flag = (16 if rng.random() < 0.5 else 0) | (256 if t else 0) | (0x8000 if rng.random() < 0.05 else 0)
            tid = int(rng.choice([0, 0, 0, 1, 2]))
            pos = c if rng.random() < 0.25 else c + int(rng.integers(-300, 301))
            kind = rng.random()
            if kind < 0.6:
                cigar, md = [(50, "M")], "50"
            elif kind < 0.8:
                cigar, md = [(20, "M"), (2, "I"), (28, "M")], "48"
            else:
                cigar, md = [(20, "M"), (3, "D"), (30, "M")], "20^ACG30"
            recs.append((flag, tid, max(pos, 0), int(rng.integers(0, 4)), cigar, md))
        per_read.append(recs)
    return pm.Records(per_read)


BATCHES = [(seed, 40) for seed in range(8)]  # 320 pairs in all


@pytest.mark.parametrize("orient", [om.FR, om.RF, om.FF])
@pytest.mark.parametrize("seed,n", BATCHES)
def test_the_direct_statement_and_the_reduction_agree(seed, n, orient):
    rng = np.random.default_rng(1000 + seed)
    res = _random_batch(rng, n)
    I, X = int(rng.integers(0, 60)), int(rng.integers(200, 500))
    v = om.virtual(res, n, orient)
    direct = om.choose(res, n, I, X, orient)
    assert direct == pm.choose(v, n, I, X)
    lines, n_proper = om.expected(res, n, I, X, orient)
    v_lines, v_proper = pm.expected(v, n, I, X)
    assert (lines, n_proper) == (om.real_lines(v_lines, orient), v_proper)
    assert n_proper >= n // 10  # (the batches do pair)
    # per combination, too: the insert of every (a, b)
    for i in range(n):
        for ja in range(int(res.rec_off[i]), int(res.rec_off[i + 1])):
            for jb in range(int(res.rec_off[n + i]), int(res.rec_off[n + i + 1])):
                assert om.insert_of(res, ja, jb, I, X, orient) == pm.insert_of(v, ja, jb, I, X)
    # the arrays' flag column is the lines'
    arrays = om.pair_arrays(res, n, I, X, orient)
    assert [int(f) for f in arrays["flag"]] == [l[2] for l in lines] and arrays["n_proper"] == n_proper
    # the estimate: directly and through insert_model on the virtual records
    assert om.estimate(res, n, orient) == im.estimate(v, n)


@pytest.mark.parametrize("seed,n", BATCHES[:3])
def test_fr_is_the_pair_model(seed, n):
    rng = np.random.default_rng(1000 + seed)
    res = _random_batch(rng, n)
    assert np.array_equal(om.virtual(res, n, om.FR).r_flag, res.r_flag)
    assert om.choose(res, n, 10, 400, om.FR) == pm.choose(res, n, 10, 400)
    assert om.expected(res, n, 10, 400, om.FR) == pm.expected(res, n, 10, 400)
    assert om.estimate(res, n, om.FR) == im.estimate(res, n)


def test_the_orientations_differ_and_tlen_follows_the_leftmost_mate():
    rng = np.random.default_rng(5)
    res = _random_batch(rng, 60)
    got = {o: om.expected(res, 60, 0, 400, o) for o in (om.FR, om.RF, om.FF)}
    assert len({repr(v) for v in got.values()}) == 3
    for o, (lines, _) in got.items():
        by_pair = {}
        for r, j, flag, mt, mp, tlen in lines:
            if flag & 2 and not flag & 256:
                by_pair.setdefault(r % 60, []).append((int(res.r_pos[j]), tlen, flag))
        for (p1, t1, f1), (p2, t2, f2) in by_pair.values():
            assert t1 == -t2 and t1 != 0
            if p1 != p2:  # +ins on the leftmost-starting mate
                assert (t1 > 0) == (p1 < p2)
            same = bool(f1 & 16) == bool(f2 & 16)
            assert same == (o == om.FF)


def test_virtual_reads_and_flags_are_involutions():
    reads = [b"ACGTN", b"AAC", b"GGT", b"TTTN"]
    for o in (om.FR, om.RF, om.FF):
        assert om.virtual_reads(om.virtual_reads(reads, 2, o), 2, o) == reads
        for flag in (0x41, 0x81 | 16, 0x41 | 0x20, 0x81 | 8, 0x41 | 4 | 0x20, 0x81 | 4 | 8):
            assert om.real_flag(om.real_flag(flag, o), o) == flag
    assert om.virtual_reads(reads, 2, om.FF) == [b"ACGTN", b"AAC", b"ACC", b"NAAA"]
    assert om.real_flag(0x81, om.FF) == 0x81 | 0x10 and om.real_flag(0x41, om.FF) == 0x41 | 0x20
    assert om.real_flag(0x41 | 8, om.RF) == 0x41 | 8 | 0x10 and om.real_flag(0x81 | 4 | 0x20, om.RF) == 0x81 | 4


# ---- the library estimate ----

def _pair(kind, ins, pos=1000, L=50):
    """One unique pair that is informative under `kind` alone with insert `ins` ("eq": equal pos0 on opposite strands, under FR
    and RF, insert L; None: under none)."""
    m = [(L, "M")]
    far = pos + ins - L
    return {om.FR: ([(0, 0, pos, 0, m, "50")], [(16, 0, far, 0, m, "50")]),
            om.RF: ([(16, 0, pos, 0, m, "50")], [(0, 0, far, 0, m, "50")]),
            om.FF: ([(0, 0, pos, 0, m, "50")], [(0, 0, far, 0, m, "50")]),
            "eq": ([(0, 0, pos, 0, m, "50")], [(16, 0, pos, 0, m, "50")]),
            None: ([(0, 0, pos, 0, m, "50")], [(16, 1, pos, 0, m, "50")])}[kind]


def _library(counts):
    """A batch of unique pairs, counts[kind] of each kind, inserts 200 + k."""
    pairs = [_pair(kind, 200 + k % 100) for kind, n in counts.items() for k in range(n)]
    res = pm.Records([p[0] for p in pairs] + [p[1] for p in pairs])
    return om.library_estimate(res, len(pairs)), len(pairs)


def test_a_clear_majority_is_chosen():
    lib, n = _library({om.FF: 300, om.FR: 120, om.RF: 80})
    assert lib["orientation"] == om.FF
    assert [e["n_informative"] for e in lib["by"]] == [120, 80, 300]
    assert all(e["n_pairs"] == n and e["n_unique"] == n and e["estimated"] for e in lib["by"])


def test_an_exact_tie_goes_to_fr_then_rf():
    assert _library({om.FR: 70, om.RF: 70, om.FF: 70})[0]["orientation"] == om.FR
    assert _library({om.FR: 69, om.RF: 70, om.FF: 70})[0]["orientation"] == om.RF
    assert _library({om.FR: 10, om.RF: 70, om.FF: 71})[0]["orientation"] == om.FF


def test_the_majority_counts_only_among_the_estimated():
    # RF, one pair short of 64, is not estimated and cannot be chosen; FR and FF tie at 64 and FR goes first
    lib, _ = _library({om.FR: 64, om.RF: 63, om.FF: 64})
    assert lib["orientation"] == om.FR and not lib["by"][om.RF]["estimated"]


def test_all_below_64_is_no_choice():
    lib, _ = _library({om.FR: 63, om.RF: 63, om.FF: 63, None: 40})
    assert lib["orientation"] == -1 and not any(e["estimated"] for e in lib["by"])
    assert all(e["min_insert"] == 0 and e["max_insert"] == 0 for e in lib["by"])
    assert _library({})[0]["orientation"] == -1


def test_an_equal_pos0_pair_counts_under_fr_and_rf():
    lib, _ = _library({"eq": 5})
    assert [e["n_informative"] for e in lib["by"]] == [5, 5, 0]
    assert lib["by"][om.FR]["q50"] == 50 and lib["by"][om.RF]["q50"] == 50
    # ... and tips a tie: 60 + 5 reach 64 under FR and RF, FF's 64 do too; FR and RF have more
    lib, _ = _library({om.FR: 60, om.RF: 60, om.FF: 64, "eq": 5})
    assert [e["n_informative"] for e in lib["by"]] == [65, 65, 64] and lib["orientation"] == om.FR
