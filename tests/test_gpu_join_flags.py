"""The flag phase and the marks of seed_join_kernel's units (fem_seed_join.hip.h, fem_seed_join_unit.hip.h; docs/NOTEBOOK.md round 11).

Since round 11 a unit's flagged values are gathered chunk by chunk in one register and compacted into the group's array when a lane
is flagged a second time and at the unit's end; lanes without an entry are told from the others by their value alone; the marks of
a slot's second value go into the word its insert addressed, and only a value in bit 0 or bit 31 of a word writes into the
neighbouring word.  What can go wrong depends on the BIT POSITION of a value's slot in its bitmap word (value mod 256: slot =
value >> 3, 32 slots per word), on the word (the table's first and last one, the guard word behind it: coordinates a multiple of
2^18 apart share a slot), on WHICH LANES hold the flagged values of a unit's lists (the same lane in two lists: a flush in between;
different lanes: one flush per unit), on their number (64 per unit) and on the order the survivors come out in.

One reference of four sequences, about 300 kbp, whose second sequence crosses 2^18 in the join's coordinates (goff[seq] + pos, with
GAP positions in front of every sequence) — in the first bank, so also where the reference is cut into banks of two sequences:
  * COPIES: a unit of 400 bases three times, the third with a 1-base, a 2-base and a 3-base deletion 130 bases apart (partners 1-3
    apart: the same or the neighbouring slot), the second across the 2^18 boundary; reads at every start offset.
  * SOLO regions as in test_gpu_join_units.py (their helpers: tests/cases.py, tests/harness.py), lists of exactly 40 and 64 entries: the true place
    sits in different lanes from list to list, the unit stays in the plain body.  Everywhere else lists have one entry: lane 0.
  * whole units of 60 bases in 32 and 40 copies: two agreeing lists flag 64 or 80 values, three more — as many as a group's array
    takes, or beyond: the read stays or goes to the generic kernel.
  * groups of 2, 3, 5 and 8 near-copies (one or two substitutions): 2-8 candidates per strand, the general survivor path.
Every batch is compared array for array with the oracle, counters included, through the padded, the compact and the banked form
of join_read; what a batch is meant to hold is asserted from the oracle before anything runs on the GPU.
Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import util
from tests.cases import SOLO_LEN, SOLO_SLOTS, lone_copies, over_home
from tests.harness import JOIN_FORMS, JoinWorld, join_check

pytestmark = pytest.mark.gpu

GAP = 2048                                 # positions in front of every sequence in the join's coordinates (kDenseGap)
PERIOD = 1 << 18                           # coordinates this far apart share a slot of the bitmap (32 Ki slots of 8 positions)
SEQ_LEN = (150_000, 120_000, 20_000, 15_000)
UNIT = 400
DELS = ((60, 1), (190, 2), (320, 3))       # the third copy: (offset in the unit, bases deleted)
SOLO = (40, 64)                            # entries of every 12-mer's list in the solo regions of class 0, 1
SOLO_HOMES = 3
WHOLE = (32, 40)                           # copies of the two whole units of 60 bases
WHOLE_LEN = 60
NEAR_GROUPS = (2, 3, 5, 8)                 # near-copies per group
NEAR_LEN = 150
FORMS = JOIN_FORMS
CASES = [(100, 3, 1), (100, 2, 1), (100, 4, 1), (150, 7, 1)]  # (L, e, a)


def _goff(sq):
    return GAP + sum(n + GAP for n in SEQ_LEN[:sq])


class _Layout:
    """A sequence under construction: pieces at chosen or at the next free positions, random bases in between."""

    def __init__(self, rng, length):
        self.rng, self.length, self.out = rng, length, bytearray()

    def skip_to(self, pos):
        assert pos >= len(self.out), (pos, len(self.out))
        self.out += util.rand_seq(self.rng, pos - len(self.out))

    def put(self, piece, gap=0):
        self.out += util.rand_seq(self.rng, gap + (-(len(self.out) + gap)) % 3)  # (pieces start at a position = 0 mod 3: the index's step)
        at = len(self.out)
        self.out += piece
        return at

    def done(self):
        assert len(self.out) <= self.length, (len(self.out), self.length)
        self.skip_to(self.length)
        return bytes(self.out)


def _build_reference():
    rng = np.random.default_rng(1116)
    unit = util.rand_seq(rng, UNIT)
    third = bytearray(unit)
    for at, n in reversed(DELS):
        del third[at:at + n]
    regions = [util.rand_seq(rng, SOLO_LEN) for _ in SOLO]
    whole = [util.rand_seq(rng, WHOLE_LEN) for _ in WHOLE]
    near = [util.rand_seq(rng, NEAR_LEN) for _ in NEAR_GROUPS]
    lone_plan = [[] for _ in SEQ_LEN]      # per sequence: (class, slot) of the 12-mers that stand alone there
    for c, n in enumerate(SOLO):
        for j in range(SOLO_SLOTS):
            for sq in rng.integers(0, len(SEQ_LEN), n - SOLO_HOMES):
                lone_plan[int(sq)].append((c, j))
    whole_plan = [[] for _ in SEQ_LEN]
    for i, n in enumerate(WHOLE):
        for sq in rng.integers(0, len(SEQ_LEN), n):
            whole_plan[int(sq)].append(i)
    copies = {"unit": [], "near": {g: [] for g in range(len(NEAR_GROUPS))}, "whole": {i: [] for i in range(len(WHOLE))},
              "home": {c: [] for c in range(len(SOLO))}}
    seqs = []
    for sq, length in enumerate(SEQ_LEN):
        lay = _Layout(rng, length)
        lay.skip_to(3000)
        if sq == 0:
            copies["unit"].append((sq, lay.put(unit, 300), "plain"))
            copies["unit"].append((sq, lay.put(bytes(third), 900), "deletions"))
        lone = [lone_plan[sq][int(j)] for j in rng.permutation(len(lone_plan[sq]))]
        lay.put(lone_copies(rng, regions, lone), 60)
        for i in [whole_plan[sq][int(j)] for j in rng.permutation(len(whole_plan[sq]))]:
            copies["whole"][i].append((sq, lay.put(whole[i], int(rng.integers(10, 60)) * 3)))
        for c in range(len(SOLO)):
            for _ in range(SOLO_HOMES if sq == c else 0):
                copies["home"][c].append((sq, lay.put(regions[c], 72)))
                lay.put(b"", 72)
        for g, n in enumerate(NEAR_GROUPS):
            for _ in range(n if sq == g % 2 else 0):  # a group stands in one sequence: one bank holds all its candidates
                piece = bytearray(near[g])
                for at in rng.choice(NEAR_LEN, int(rng.integers(1, 3)), replace=False):
                    piece[at] = util.ACGT[(np.searchsorted(util.ACGT, piece[at]) + 1 + rng.integers(0, 3)) % 4]
                copies["near"][g].append((sq, lay.put(bytes(piece), 200)))
        if sq == 1:
            # the unit once more, so that the read starts drawn around it (60 bases before .. 60 behind) cross the 2^18 boundary
            # of the join's coordinates about in their middle
            at = PERIOD - _goff(1) - 150
            at -= at % 3
            lay.skip_to(at)
            copies["unit"].append((sq, lay.put(unit), "plain"))
        seqs.append(lay.done())
    return seqs, copies


class _World(JoinWorld):
    def __init__(self):
        self.seqs, self.copies = _build_reference()
        assert tuple(len(s) for s in self.seqs) == SEQ_LEN and sum(SEQ_LEN) > PERIOD and sum(SEQ_LEN) < 320_000
        (sq, pos, _), = [c for c in self.copies["unit"] if c[0] == 1]
        assert _goff(sq) + pos - 60 < PERIOD - 8 and PERIOD + 8 < _goff(sq) + pos + UNIT - 150 + 60
        self.ref = fo.Reference(self.seqs)
        self.idx = fo.OracleIndex(self.ref)
        self._lists()
        self.devices, self.wanted = {}, {}

    def _lists(self):
        """From the oracle's index: the solo regions' and the whole units' lists are exactly as long as planned, and the bulk of the
        reference has lists of one entry."""
        freq = np.diff(self.idx.lookup.astype(np.int64))
        assert np.count_nonzero(freq == 1) > 0.9 * np.count_nonzero(freq)
        for n in SOLO:
            assert np.count_nonzero(freq == n) >= SOLO_SLOTS, (n, np.count_nonzero(freq == n))
        for n in WHOLE:
            assert np.count_nonzero(freq == n) >= WHOLE_LEN // 3 - 4, (n, np.count_nonzero(freq == n))
        for c in range(len(SOLO)):
            assert len(self.copies["home"][c]) == SOLO_HOMES


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _substitute(rng, s, k):
    s = bytearray(s)
    for at in rng.choice(len(s), k, replace=False):
        s[at] = util.ACGT[(np.searchsorted(util.ACGT, s[at]) + 1 + rng.integers(0, 3)) % 4]
    return bytes(s)


def _reads_at_every_offset(w, seed, L, e, reps=3):
    """Reads of L bases with e substitutions at every start offset from 60 bases before each copy of the unit to where the read ends 60
    bases behind it, `reps` times on each strand."""
    rng = np.random.default_rng(seed)
    reads, starts = [], []
    for sq, pos, _ in w.copies["unit"]:
        for start in range(pos - 60, pos + UNIT - L + 60 + 1):
            for _ in range(reps):
                r = _substitute(rng, w.seqs[sq][start:start + L], e)
                reads += [r, util.revcomp(r)]
                starts.append(_goff(sq) + start)
    return reads, np.array(starts)


def _accepted(want, e):
    """-> per accepted candidate (one that verification kept): its coordinate in the join (first bank or no banks; the oracle
    reports the candidate e before it), its strand"""
    n_strands = len(want.cand_off) - 1
    strand = np.repeat(np.arange(n_strands) & 1, np.diff(want.cand_off.astype(np.int64)))
    goff = np.array([_goff(i) for i in range(len(SEQ_LEN))], dtype=np.int64)
    v = goff[(want.cands >> np.uint64(32)).astype(np.int64)] + (want.cands & np.uint64(0xFFFFFFFF)).astype(np.int64) + e
    ok = want.v_ed != 0xFF
    return v[ok], strand[ok]


def _want(w, key, make, e, a):
    if key not in w.wanted:
        reads, about = make()
        batch = fo.ReadBatch(reads)
        w.wanted[key] = (batch, fo.map_reads(w.ref, w.idx, batch, e=e, a=a, threads=8), about)
    return w.wanted[key]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L,e,a", CASES)
def test_every_bit_position_of_a_slot_and_the_word_edges(world, L, e, a, form):
    batch, want, starts = _want(world, ("offsets", L, e, a), lambda: _reads_at_every_offset(world, 31 * e + L, L, e), e, a)
    assert np.bincount(starts % 256, minlength=256).min() >= 8, "reads drawn per residue of the start, on each strand"
    # by the oracle: mapped reads in every residue class of the candidate coordinate mod 256 (32 bit positions x 8 positions of a
    # slot) on both strands, and at every coordinate within 8 of the 2^18 boundary (slots 32 767 and 0: the table's last word with
    # the guard word behind it, the first word).  The copy with the deletions gives every read over one a partner 1-3 positions away.
    v, strand = _accepted(want, e)
    for s in (0, 1):
        per_class = np.bincount(v[strand == s] % 256, minlength=256)
        assert per_class.min() >= 1, (s, int(per_class.argmin()))
        d = v[strand == s] - PERIOD
        near_edge = np.bincount(d[(d >= -8) & (d < 8)] + 8, minlength=16)
        assert near_edge.min() >= 1, (s, near_edge)
    per_strand = np.diff(want.cand_off.astype(np.int64))
    assert np.count_nonzero(per_strand >= 2) > 0.5 * batch.n, "reads over the copies have a candidate in each"
    join_check(world, form, batch, want, e, a)


def _over(rng, w, sq, pos, n, L, e):
    """A read of L bases over the piece of n bases at (sq, pos), 0..e edits, either strand."""
    s = w.seqs[sq]
    start = max(0, min(len(s) - L - e - 1, pos - int(rng.integers(0, max(1, L - n + 1))) if n <= L else pos + int(rng.integers(0, n - L + 1))))
    r = util.mutate(rng, s[start:start + L + e], int(rng.integers(0, e + 1)))[:L]
    r = r + util.rand_seq(rng, L - len(r))
    return util.revcomp(r) if rng.random() < 0.5 else r


def _lanes_batch(w, seed, L, e):
    """-> reads: random ones (lists of one entry: lane 0), over the whole units of 32 and 40 copies, over the groups of near-copies,
    then over the solo regions; (where the solo reads begin, the class of each)"""
    rng = np.random.default_rng(seed)
    reads = util.make_reads(rng, w.seqs, 1200, L, e)
    for i in range(len(WHOLE)):
        places = w.copies["whole"][i]
        reads += [_over(rng, w, *places[int(j)], WHOLE_LEN, L, e) for j in rng.integers(0, len(places), 150)]
    for g in range(len(NEAR_GROUPS)):
        places = w.copies["near"][g]
        reads += [_over(rng, w, *places[int(j)], NEAR_LEN, L, e) for j in rng.integers(0, len(places), 120)]
    first, cls = len(reads), []
    for c in range(len(SOLO)):
        for sq, pos in w.copies["home"][c]:
            for _ in range(60):
                r = over_home(rng, w, c, sq, pos, L, e)
                reads.append(util.revcomp(r) if rng.random() < 0.5 else r)
                cls.append(c)
    return reads, (first, np.array(cls))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L,e,a", CASES)
def test_flagged_lanes_capacity_and_survivor_order(world, L, e, a, form):
    batch, want, (first, cls) = _want(world, ("lanes", L, e, a), lambda: _lanes_batch(world, 53 * e + L, L, e), e, a)
    per_strand = np.diff(want.cand_off.astype(np.int64)).reshape(-1, 2)
    pre = want.pre.astype(np.int64).reshape(-1, 2)
    R = e + 1 + a
    # lanes: reads over a solo region that picked a seed of it (the sum of the selected frequencies reaches the class's list
    # length: the other lists of such a read have one entry, at most 3 x 10 of them) and have few candidates — join_read keeps them,
    # in its plain body (no list beyond 64 entries), with the three true places in lanes that differ from list to list.  At R = 4
    # the selection can step over a region (test_gpu_join_units.py): 20 % there, 80 % otherwise.
    n = len(cls)
    solo_ok = (pre[first:first + n].max(axis=1) >= np.array(SOLO)[cls]) & (per_strand[first:first + n].max(axis=1) < 16) & (per_strand[first:first + n].max(axis=1) >= 1)
    for c in range(len(SOLO)):
        drawn = np.count_nonzero(cls == c)
        assert np.count_nonzero(solo_ok & (cls == c)) >= (0.8 if R >= 5 else 0.2) * drawn, (SOLO[c], np.count_nonzero(solo_ok & (cls == c)), drawn)
    # capacity: strands with 32 and with 40 candidates — two agreeing lists flag 64 and 80 values, three 96 and 120: at the cap of
    # a group's array (64 at R <= 6) and beyond it; such a read stays or goes to the generic kernel, and both must equal the oracle
    # (at R = 4 the selection steps over a unit of 60 bases into the flanks' lists of one entry: no such strand there)
    for copies in WHOLE if R >= 5 else ():
        assert np.count_nonzero(per_strand.max(axis=1) == copies) >= 20, (copies, np.bincount(per_strand.max(axis=1)))
    # order: strands with 2-8 candidates (near-copies: survivors of several groups, sorted into lanes and merged; values that
    # several lists hold alike tie on the lane)
    assert np.count_nonzero((per_strand >= 2) & (per_strand <= 8)) >= 200, np.bincount(per_strand.ravel())[:10]
    for k in (2, 3, 5, 8):
        assert np.count_nonzero(per_strand == k) >= 10, (k, np.bincount(per_strand.ravel())[:10])
    join_check(world, form, batch, want, e, a)
