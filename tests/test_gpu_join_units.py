"""The two bodies of a unit in seed_join_kernel's join_read (fem_seed_join.hip.h), each side of the test that picks one.

A (strand, group) unit takes the PLAIN body when none of its lists has more than 64 entries and its first chunks hold no
remapped near-start entry, the FULL body otherwise.  The references of the other dense tests mostly make plain units; this one
plants short repeats with chosen copy counts — lists of exactly 60, 64, 65, 100, 128 and 129 entries — copies within the
first 1024 positions of a sequence (remapped entries), also behind entry 64 of a long list (a remapped entry in a second
chunk), and reads that change from one body to the other from unit to unit.  Every batch is compared array for array with the
oracle, through the three instances of join_read: the padded strided table, the compact table and the reference in banks.

Two kinds of repeat.  WHOLE units (60 bases copied as one piece): every seed a read picks inside one has the same places in its
list, so two such lists flag more values than a group's array takes (64) and the join hands the read to the generic kernel — the
lists of every length exist, and that hand-over is compared too, but those reads say little about the full body.  SOLO regions
(51 bases = 14 indexed 12-mers, each 12-mer copied ON ITS OWN to places of its own, the region itself in three places): wide
enough that the seed selection cannot step over one, so a read over a region picks a seed whose list has 64, 65, 100 or 128
entries, while the lists agree at the three regions only — few flagged values, three candidates: join_read finishes the read in
its full body.  Which reads do that is asserted from the oracle (selected frequencies, candidates per strand) before anything
runs on the GPU.
Needs a GPU: -m gpu."""
import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import util
from tests.cases import SOLO_LEN, SOLO_SLOTS, lone_copies, over_home
from tests.harness import JOIN_FORMS, JoinWorld, join_check

pytestmark = pytest.mark.gpu

UNIT = 60                                  # bases of a planted unit (a multiple of 3)
COUNTS = (60, 64, 65, 100, 128, 129)       # copies of units 0..5: lists of exactly that many entries
NEAR = (0, 1, 3, 17, 1000, 1023, 1024)     # starts of the near-start unit's copies (one sequence each, in turn)
N_SEQ = 4
SOLO = (64, 65, 100, 128)                  # entries of every 12-mer's list in the solo regions of class 0..3
SOLO_HOMES = 3                             # places where a region stands whole (the other entries: the 12-mer alone)


def _build_reference():
    """Four sequences of a few tens of kbp.  Every copy of units 0..5 starts at a position = 0 mod 3 (the index's step), so each of a
    unit's UNIT / 3 - 3 indexed 12-mers has a list of exactly COUNTS[i] entries.  -> sequences, {unit: [(seq, pos)]}"""
    rng = np.random.default_rng(6465)
    units = [util.rand_seq(rng, UNIT) for _ in COUNTS]
    near_unit = util.rand_seq(rng, UNIT)
    # which sequence a copy goes to: unit 3 (100 copies) has 70 copies in sequences 0-1, then one at position 300 of sequence 2
    # (remapped, and behind entry 64 of its lists), the rest behind it
    plan = [[] for _ in range(N_SEQ)]       # per sequence: units in the order they are laid down
    for i, c in enumerate(COUNTS):
        if i == 3:
            where = [0] * 35 + [1] * 35 + [2] * 15 + [3] * 14  # (+ the one at 300 of sequence 2)
        else:
            where = [int(x) for x in rng.integers(0, N_SEQ, c)]
        for s in where:
            plan[s].append(i)
    seqs, copies = [], {i: [] for i in range(len(COUNTS))}
    copies["near"] = []
    # solo regions: class c has SOLO[c] entries per 12-mer = SOLO_HOMES whole regions (sequences 0, 0, 1) + the 12-mer alone.  For
    # the classes of 100 and 128: 70 and 90 entries in the earlier sequences, then one within the first 1024 positions of
    # sequence 2 and 3 (a remapped entry in the list's SECOND chunk), the rest behind it
    regions = [util.rand_seq(rng, SOLO_LEN) for _ in SOLO]
    home_plan = [[2] * len(SOLO), [1] * len(SOLO), [0] * len(SOLO), [0] * len(SOLO)]
    lone_plan = [[] for _ in range(N_SEQ)]
    head_lone = {2: [], 3: []}              # sequence -> (class, slot) of the near-start copies
    for c, n in enumerate(SOLO):
        for j in range(SOLO_SLOTS):
            n_lone = n - SOLO_HOMES
            if n == 100:
                where = [0] * 33 + [1] * 34 + [3] * (n_lone - 68)   # 2 + 33 | 1 + 34 = 70 entries before sequence 2
                head_lone[2].append((c, j))
            elif n == 128:
                where = [0] * 30 + [1] * 30 + [2] * 27 + [3] * (n_lone - 88)  # 90 entries before sequence 3
                head_lone[3].append((c, j))
            else:
                where = [int(x) for x in rng.integers(0, N_SEQ, n_lone)]
            for sq in where:
                lone_plan[sq].append((c, j))
    for c in range(len(SOLO)):
        copies[("home", c)] = []
    for s in range(N_SEQ):
        order = [plan[s][int(j)] for j in rng.permutation(len(plan[s]))]
        out = bytearray()
        # the first 1100 positions: the near-start unit's copies of this sequence, unit 3 at 300 of sequence 2
        head = {at: near_unit for j, at in enumerate(NEAR) if j % N_SEQ == s}
        if s == 2:
            head[300] = units[3]
        if s in head_lone:                                      # 12-mers of the solo regions, alone, behind the near-start unit
            head[63 if s == 2 else 78] = head_lone[s]
        assert 63 + 12 + 15 * SOLO_SLOTS + 15 <= 300
        for at in sorted(head):
            out += util.rand_seq(rng, at - len(out))
            if isinstance(head[at], list):
                out += lone_copies(rng, regions, head[at])
                continue
            out += head[at]
            copies["near" if head[at] is near_unit else 3].append((s, at))
        out += util.rand_seq(rng, 1101 - len(out))  # (1101 = 0 mod 3)
        for i in order:
            gap = int(rng.integers(0, 4)) * 3 if rng.random() < 0.4 else int(rng.integers(10, 60)) * 3  # short gaps: reads over two copies
            out += util.rand_seq(rng, gap)
            copies[i].append((s, len(out)))
            out += units[i]
        for _ in range(6):                  # the near-start unit again, far from the start, in all three phases
            out += util.rand_seq(rng, int(rng.integers(100, 200)))
            copies["near"].append((s, len(out)))
            out += near_unit
        # SOLO regions.  The 12-mers alone, each followed by three bases chosen so that no indexed 12-mer across the joint is one of
        # the region's again (the lists stay exactly as long as planned), then this sequence's whole regions between flanks
        out += util.rand_seq(rng, (-len(out)) % 3)
        lone = [lone_plan[s][int(j)] for j in rng.permutation(len(lone_plan[s]))]
        out += lone_copies(rng, regions, lone)
        for c in range(len(SOLO)):
            for _ in range(home_plan[s][c]):
                out += util.rand_seq(rng, 72)
                copies[("home", c)].append((s, len(out)))
                out += regions[c]
                out += util.rand_seq(rng, 72 + (-SOLO_LEN) % 3)
        out += util.rand_seq(rng, int(rng.integers(3000, 5000)))  # a plain stretch
        seqs.append(bytes(out))
    # MIRRORS: the surroundings of the whole solo regions of the long classes once more, reverse-complemented, behind the plain
    # stretches.  A read drawn there finds a long list on one strand and lists of one entry on the other.
    copies["mirrored"] = []
    for s in range(N_SEQ):
        out = bytearray(seqs[s])
        for c in range(1, len(SOLO)):
            for sq, pos in copies[("home", c)]:
                if (sq + pos) % N_SEQ != s:
                    continue
                copies["mirrored"].append((c, sq, pos))
                out += util.revcomp(seqs[sq][pos - 60:pos + SOLO_LEN + 60]) + util.rand_seq(rng, int(rng.integers(20, 90)))
        seqs[s] = bytes(out + util.rand_seq(rng, 400))
    return seqs, copies


def _list_classes(idx):
    """What the test stands on, from the oracle's index: the planted lists exist in every class of length, a remapped entry
    sits in the second chunk of a list, every sequence has a planted copy near its start."""
    freq = np.diff(idx.lookup.astype(np.int64))
    for c in COUNTS:
        assert np.count_nonzero(freq == c) >= UNIT // 3 - 4, (c, np.count_nonzero(freq == c))
    assert np.count_nonzero(freq <= 64) and np.count_nonzero((freq > 64) & (freq <= 128)) and np.count_nonzero(freq > 128)
    in_second = 0
    for h in np.nonzero((freq > 64) & (freq <= 128))[0]:
        tail = idx.occ[int(idx.lookup[h]) + 64:int(idx.lookup[h + 1])]
        in_second += int(np.count_nonzero((tail & np.uint64(0xFFFFFFFF)) < np.uint64(1024)))
    assert in_second >= 10, in_second


def _solo_lists(w):
    """Every indexed 12-mer of every whole solo region has a list of exactly its class's length; in the classes of 100 and 128 an
    entry of the list's second chunk (index >= 64) lies within the first 1024 positions of its sequence."""
    order = np.argsort(w.idx.occ[:w.idx.n_occ], kind="stable")
    for c, n in enumerate(SOLO):
        assert len(w.copies[("home", c)]) == SOLO_HOMES
        for sq, pos in w.copies[("home", c)]:
            assert pos % 3 == 0 and w.seqs[sq][pos:pos + SOLO_LEN] == w.seqs[w.copies[("home", c)][0][0]][w.copies[("home", c)][0][1]:][:SOLO_LEN]
            for j in range(SOLO_SLOTS):
                key = np.uint64((sq << 32) | (pos + 3 * j))
                at = int(order[np.searchsorted(w.idx.occ[:w.idx.n_occ], key, sorter=order)])
                assert w.idx.occ[at] == key
                h = int(np.searchsorted(w.idx.lookup, np.uint32(at), side="right")) - 1  # (the bucket that holds entry `at`)
                lst = w.idx.occ[int(w.idx.lookup[h]):int(w.idx.lookup[h + 1])]
                assert len(lst) == n, (c, j, len(lst))
                if n in (100, 128):
                    assert np.count_nonzero((lst[64:] & np.uint64(0xFFFFFFFF)) < np.uint64(1024)) == 1, (c, j)


class _World(JoinWorld):
    def __init__(self):
        self.seqs, self.copies = _build_reference()
        assert len(self.copies["mirrored"]) == SOLO_HOMES * (len(SOLO) - 1)
        assert all(20_000 < len(s) < 70_000 for s in self.seqs) and sum(len(s) for s in self.seqs) < 200_000
        for i, c in enumerate(COUNTS):
            assert len(self.copies[i]) == c and all(pos % 3 == 0 for _, pos in self.copies[i])
        for s in range(N_SEQ):
            assert any(sq == s and pos < 1024 for sq, pos in self.copies["near"]), s
        self.ref = fo.Reference(self.seqs)
        self.idx = fo.OracleIndex(self.ref)
        _list_classes(self.idx)
        _solo_lists(self)
        self.devices, self.wanted = {}, {}


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _over_copy(rng, w, sq, pos, L, e):
    """A read of L bases that covers the copy at (sq, pos), with 0..e edits, on either strand."""
    s = w.seqs[sq]
    start = max(0, min(len(s) - L - e - 1, pos - int(rng.integers(0, L - UNIT + 1))))
    r = util.mutate(rng, s[start:start + L + e], int(rng.integers(0, e + 1)))[:L]
    r = r + util.rand_seq(rng, L - len(r))
    return util.revcomp(r) if rng.random() < 0.5 else r


def _reads(w, seed, L, e, n_random=1400):
    rng = np.random.default_rng(seed)
    reads = util.make_reads(rng, w.seqs, n_random, L, e)  # across the copies and the plain stretches
    for key, places in w.copies.items():
        if key == "mirrored" or isinstance(key, tuple):
            continue
        picks = places if key == "near" else [places[int(j)] for j in rng.integers(0, len(places), 140)]
        reads += [_over_copy(rng, w, sq, pos, L, e) for sq, pos in picks]
    for s in w.seqs:  # the very first positions of every sequence: remapped entries, entries dropped for pos < start
        for at in NEAR:
            reads += [s[at:at + L], util.revcomp(s[at:at + L])]
    return reads


def _solo_reads(w, seed, L, e, n_per_home=60):
    """-> reads over the whole solo regions (either strand), the class of each"""
    rng = np.random.default_rng(seed)
    reads, cls = [], []
    for c in range(len(SOLO)):
        for sq, pos in w.copies[("home", c)]:
            for _ in range(n_per_home):
                r = over_home(rng, w, c, sq, pos, L, e)
                reads.append(util.revcomp(r) if rng.random() < 0.5 else r)
                cls.append(c)
    return reads, np.array(cls)


def _finished_in_the_full_body(want, cls, first, long_classes=(1, 2, 3)):
    """Reads first.. of the batch (classes cls) that, by the oracle, picked a seed with a list of 65-128 entries AND have fewer than
    16 candidates on either strand.  The sum of the selected seeds' frequencies (`pre`) reaches the class's list length only if
    a seed of the region was picked: every other list a read over a solo region can pick has one to three entries (at most 3 x
    10 picked seeds).  What a unit flags is about two values per candidate (a pair within e) + the chance flags, about
    3 n^2 / 32768 slots for n entries in the unit: 2 to 14 for one to three such lists.  Below 16 candidates that stays under
    join_read's limits (64 flagged values per unit, 64 candidates per strand): it keeps the read.  -> their number per class"""
    n = len(cls)
    pre = want.pre.astype(np.int64).reshape(-1, 2)[first:first + n]
    per_strand = np.diff(want.cand_off.astype(np.int64)).reshape(-1, 2)[first:first + n]
    need = np.array(SOLO)[cls]
    ok = (pre.max(axis=1) >= need) & (per_strand.max(axis=1) < 16) & (per_strand.max(axis=1) >= 1)
    return {c: int(np.count_nonzero(ok & (cls == c))) for c in long_classes}, ok


# e = 2, 3, 4: R = 4, 5, 6 (seven waves per SIMD); 150 bases at e = 7: R = 9 (the kernels of six waves per SIMD); a = 2 once
CASES = [(2, 1, 100), (3, 1, 100), (4, 1, 100), (7, 1, 150), (3, 2, 100)]


def _main_batch(w, e, a, L):
    reads = _reads(w, 100 * e + a, L, e)
    solo, cls = _solo_reads(w, 7000 + 100 * e + a, L, e)
    return reads + solo, (len(reads), cls)


def _want(w, key, make, e, a):
    """The oracle's result of a batch, made once and shared by the three forms, + what its maker says about the reads."""
    if key not in w.wanted:
        reads, about = make()
        batch = fo.ReadBatch(reads)
        w.wanted[key] = (batch, fo.map_reads(w.ref, w.idx, batch, e=e, a=a, threads=8), about)
    return w.wanted[key]


@pytest.mark.parametrize("form", list(JOIN_FORMS))
@pytest.mark.parametrize("e,a,L", CASES)
def test_lists_on_both_sides_of_the_split_equal_the_oracle(world, e, a, L, form):
    batch, want, (first, cls) = _want(world, (e, a, L), lambda: _main_batch(world, e, a, L), e, a)
    assert 2000 <= batch.n <= 4000
    assert want.stats[1] > 0.7 * batch.n
    assert np.diff(want.cand_off.astype(np.int64)).max() >= 60, "whole units: strands the join hands to the generic kernel"
    # reads the join finishes in its full body, by class of list length.  A region of 14 consecutive seeds of one phase group
    # cannot be stepped over when the selection's freedom (columns of its table: seeds of a group - 4 R + 1) is below 14: R >= 5
    # at these lengths; at R = 4 (15 columns) one offset of the region in four forces a seed into it.  Edits inside a region and
    # reads whose other picks add candidates take some away: 80 % and 20 % of the reads drawn per class.
    done, _ = _finished_in_the_full_body(want, cls, first)
    drawn = np.count_nonzero(cls == 1)
    R = e + 1 + a
    for c, n in done.items():
        assert n >= (0.8 if R >= 5 else 0.2) * drawn, (SOLO[c], n, drawn)
    # ... and on the other side of the boundary: lists of exactly 64 entries, kept by the join too (plain body)
    short, _ = _finished_in_the_full_body(want, cls, first, long_classes=(0,))
    assert short[0] >= (0.8 if R >= 5 else 0.2) * drawn, short
    join_check(world, form, batch, want, e, a)


def _two_bodies_in_one_read(w, seed, L=100, e=3):
    """Reads over the mirrored solo regions (_build_reference): on the forward strand a unit with a list of 65, 100 or 128 entries
    (full body), on the reverse strand, whose units come behind it in the kernel's loop, the mirror's lists of one entry (plain
    body) — and each read reverse-complemented too, where the plain unit comes first.  -> reads, (0, class of each)"""
    rng = np.random.default_rng(seed)
    reads, cls = [], []
    for n in range(1000):
        c, sq, pos = w.copies["mirrored"][n % len(w.copies["mirrored"])]
        r = over_home(rng, w, c, sq, pos, L, e)
        reads += [r, util.revcomp(r)]
        cls += [c, c]
    return reads, (0, np.array(cls))


@pytest.mark.parametrize("form", list(JOIN_FORMS))
def test_a_unit_of_one_body_after_a_unit_of_the_other(world, form):
    # state must not leak from unit to unit: the bitmap clean, nothing left of a second chunk or of the survivors' masks
    e, a = 3, 1
    batch, want, (first, cls) = _want(world, "two bodies", lambda: _two_bodies_in_one_read(world, 77), e, a)
    # by the oracle: a long list picked on one strand, none on the other, candidates on BOTH strands and few of them — the
    # join keeps the read and runs a full and a plain unit in it, in this order in every second read and in the other in the rest
    _, ok = _finished_in_the_full_body(want, cls, first)
    pre = want.pre.astype(np.int64).reshape(-1, 2)
    per_strand = np.diff(want.cand_off.astype(np.int64)).reshape(-1, 2)
    both = ok & (pre.min(axis=1) < 65) & (pre.min(axis=1) >= 2) & (per_strand.min(axis=1) >= 1)
    full_first = both & (pre[:, 0] > pre[:, 1])
    assert np.count_nonzero(full_first) >= 0.3 * batch.n and np.count_nonzero(both & ~full_first) >= 0.3 * batch.n, (np.count_nonzero(full_first), np.count_nonzero(both))
    join_check(world, form, batch, want, e, a)
