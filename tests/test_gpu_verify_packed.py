"""verify_kernel_packed (fem_amd/csrc/fem_verify.hip.h): a batch that came packed — equal-length reads at two bits per
base — is verified straight from its codes; reads with anything but upper-case ACGT take their characters.  Every batch
here is staged packed (pack_reads -> commit_stage_packed) and compared array for array with the oracle and with a second
handle on which FEM_VERIFY_CHARS=1 keeps the character kernel (verify_kernel) on the same packed batch.

The lengths sit on every boundary of the kernel's read side: one 16-column step and its partial form, the 64-column
stretch of one 16-byte load with the reverse strand's funnel shift at each L mod 4, the planes' 96-column stretch, and
reads that are streamed over many stretches.  A read needs (e + 2) * ceil(k / step) seeds in its smallest phase group to
get candidates at all (src/filter.c:5-7, :168-172): k = 12, step = 3 asks for 13 + 12 (e + 2) bases, so the shorter cases
run on an index of the same reference with shorter seeds (_index_of) — the verification does not see k.
Needs a GPU: -m gpu."""
import os

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests.cases import UNIT, UNIT_COPIES, packed_exceptions, packed_reads, packed_reference
from tests.harness import device_with_env, run_packed

pytestmark = pytest.mark.gpu

# (L, e): every length with one e of {0, 1, 3, 7}; a = 1 throughout
CASES = [(12, 0), (15, 1), (16, 0), (17, 0), (31, 1), (32, 3), (33, 0), (63, 7), (64, 3), (65, 1), (66, 7), (67, 3),
         (95, 7), (96, 3), (97, 1), (100, 3), (127, 7), (128, 0), (129, 3), (150, 7), (255, 3), (256, 7), (257, 1),
         (301, 3), (1024, 7)]
SWEEP = {16: 0, 63: 7, 100: 3}          # lengths that also run at the small batch sizes
SWEEP_SIZES = (1, 63, 64, 65, 257)
N_READS = 2000


def _index_of(L, e):
    """The longest seeds with which a read of L bases gets candidates at e errors and a = 1 (seed_candidates, oracle)."""
    R = e + 2
    for k, step in ((12, 3), (8, 4), (6, 3), (5, 5), (4, 4), (3, 3)):
        n_seeds, lg = L - k + 1, -(-k // step)
        if n_seeds > 0 and R <= n_seeds // step and (n_seeds - (step - 1)) // step >= R * lg:
            return k, step
    raise AssertionError("no index for L = %d, e = %d" % (L, e))


class _World:
    def __init__(self):
        rng = np.random.default_rng(20260117)
        self.seqs, self.places = packed_reference(rng)
        self.ref = fo.Reference(self.seqs)
        self.idx = {}
        self.devs = {}

    def index(self, k, step):
        if (k, step) not in self.idx:
            self.idx[(k, step)] = fo.OracleIndex(self.ref, k, step)
        return self.idx[(k, step)]

    def dev(self, k, step, chars, dense=False):
        """A handle with the (k, step) index of the reference; chars: under FEM_VERIFY_CHARS=1; dense: FEM_FORCE_DENSE=1."""
        key = (k, step, chars, dense)
        if key not in self.devs:
            switches = {"FEM_VERIFY_CHARS": chars, "FEM_FORCE_DENSE": dense}
            for name in switches:
                assert os.environ.get(name, "0") == "0", name
            d = device_with_env(**{name: "1" for name, on in switches.items() if on})
            idx = self.index(k, step)
            d.upload_reference(self.seqs)
            d.upload_index(k, step, idx.lookup, idx.occ[:idx.n_occ])
            self.devs[key] = d
        return self.devs[key]

    def close(self):
        for d in self.devs.values():
            d.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _oracle(world, reads, e, k, step):
    return fo.map_reads(world.ref, world.index(k, step), fo.ReadBatch(reads), e=e, k=k, step=step,
                        stages=fo.STAGE_SEED | fo.STAGE_VERIFY)


def _strand_has(want, read, strand, accepted=True):
    lo, hi = int(want.cand_off[2 * read + strand]), int(want.cand_off[2 * read + strand + 1])
    ed = want.v_ed[lo:hi]
    return bool(np.any(ed != 255)) if accepted else bool(np.any(ed == 255))


def _assert_mix(want, n):
    """The case holds what the kernel can get wrong: accepted candidates on both strands, rejected ones, and reads 0 and
    n - 1 accepted on the reverse strand."""
    strand = np.repeat(np.arange(2 * n) & 1, np.diff(want.cand_off.astype(np.int64)))
    ok = want.v_ed != 255
    assert np.any(ok & (strand == 0)) and np.any(ok & (strand == 1)), "accepted candidates on both strands"
    assert np.any(~ok), "rejected candidates"
    assert _strand_has(want, 0, 1) and _strand_has(want, n - 1, 1), "reads 0 and n - 1 accepted on the reverse strand"


def _check(world, reads, L, e, want=None, dense=False):
    k, step = _index_of(L, e)
    want = want or _oracle(world, reads, e, k, step)
    off, cand, ed, end, stats = run_packed(world.dev(k, step, False, dense), reads, L, e, k, step)
    assert np.array_equal(off, want.cand_off) and np.array_equal(cand, want.cands)
    assert np.array_equal(ed, want.v_ed)
    assert np.array_equal(end[ed != 255], want.v_end[want.v_ed != 255])
    off_c, cand_c, ed_c, end_c, stats_c = run_packed(world.dev(k, step, True, dense), reads, L, e, k, step)
    assert np.array_equal(off, off_c) and np.array_equal(cand, cand_c)
    assert np.array_equal(ed, ed_c) and np.array_equal(end, end_c)
    assert np.array_equal(stats, stats_c) and len(stats) == 5
    assert np.array_equal(stats, want.stats)
    return off, cand, ed, end


@pytest.mark.parametrize("L,e", CASES)
def test_every_boundary_length_against_the_oracle_and_the_character_kernel(world, L, e):
    rng = np.random.default_rng(1000 * L + e)
    k, step = _index_of(L, e)
    reads = packed_reads(rng, world.seqs, world.places, N_READS, L, e)
    want = _oracle(world, reads, e, k, step)
    _assert_mix(want, N_READS)
    _check(world, reads, L, e, want)
    # the same batch with about 3 % of its reads carrying other characters: their lanes take the characters
    odd, kind = packed_exceptions(rng, reads, 0.03)
    assert np.any(kind == 1) and np.any(kind == 2)
    _check(world, odd, L, e)


@pytest.mark.parametrize("L", sorted(SWEEP))
@pytest.mark.parametrize("n", SWEEP_SIZES)
def test_small_batches_load_at_the_buffers_edges(world, L, n):
    e = SWEEP[L]
    rng = np.random.default_rng(77 * L + n)
    k, step = _index_of(L, e)
    reads = packed_reads(rng, world.seqs, world.places, n, L, e)
    want = _oracle(world, reads, e, k, step)
    # read 0 (nothing but padding in front of its codes) and read n - 1 (nothing but slack behind) on the reverse strand
    assert _strand_has(want, 0, 1) and _strand_has(want, n - 1, 1)
    _check(world, reads, L, e, want)
    odd, _ = packed_exceptions(rng, reads, 0.03 if n > 1 else 0.0)
    _check(world, odd, L, e)


def test_a_batch_in_which_every_read_is_an_exception(world):
    L, e = 100, 3
    rng = np.random.default_rng(5)
    reads = packed_reads(rng, world.seqs, world.places, 1500, L, e)
    odd, kind = packed_exceptions(rng, reads, 1.0)
    assert np.all(kind > 0) and np.any(kind == 1) and np.any(kind == 2)
    off, cand, ed, end = _check(world, odd, L, e)  # (a read with N or R: what the oracle gives)
    # a read whose only odd characters are lower-case bases gives what its upper-case form gives
    off_u, cand_u, ed_u, end_u = _check(world, [r.upper() if kd == 1 else r for r, kd in zip(odd, kind)], L, e)
    assert np.array_equal(off, off_u)
    for r in np.flatnonzero(kind == 1):
        lo, hi = int(off[2 * r]), int(off[2 * r + 2])
        assert np.array_equal(cand[lo:hi], cand_u[lo:hi]) and np.array_equal(ed[lo:hi], ed_u[lo:hi])
        assert np.array_equal(end[lo:hi], end_u[lo:hi])


@pytest.mark.parametrize("L,e", [(65, 1), (100, 3)])
def test_groups_of_eight_inside_the_twelve_copy_unit(world, L, e):
    # reads inside the unit: 12 candidates per strand and more with the near-copies, of which whole groups of eight carry
    # the 16-bit mask (kMeta16) and the rest the 32-bit one
    rng = np.random.default_rng(800 + L)
    units = [p for p in world.places if p[2] == UNIT]
    assert len(units) == UNIT_COPIES
    reads = packed_reads(rng, world.seqs, units, 600, L, e) + packed_reads(rng, world.seqs, [], 600, L, e)
    n = len(reads)
    assert _index_of(L, e) == (12, 3)
    want = _oracle(world, reads, e, 12, 3)
    counts = np.diff(want.cand_off.astype(np.int64))
    assert np.any((counts >= 8) & (counts <= 15)) and np.any((counts > 0) & (counts < 8))
    _assert_mix(want, n)
    _check(world, reads, L, e, want)


@pytest.mark.parametrize("dense", [True, False])
def test_dense_and_sparse_index_paths(world, dense):
    # the verification is shared; the order of the candidate slots differs
    L, e = 100, 3
    rng = np.random.default_rng(31 + dense)
    reads = packed_reads(rng, world.seqs, world.places, 3000, L, e)
    want = _oracle(world, reads, e, 12, 3)
    _assert_mix(want, len(reads))
    d = world.dev(12, 3, False, dense)
    assert (d.seed_kernel(e=e) == "seed_join_kernel") == dense
    _check(world, reads, L, e, want, dense=dense)
    odd, _ = packed_exceptions(rng, reads, 0.03)
    _check(world, odd, L, e, dense=dense)


MIXED_LENGTHS = (31, 32, 33, 63, 64, 65, 95, 96, 97, 129)


def test_mixed_lengths_staged_as_characters(world):
    # one batch of every length around the 16-, 64- and 96-column boundaries, shuffled so that the lanes of a wave walk
    # different numbers of steps, sent as characters: verify_kernel with its read_off gathers, on the step it shares with the
    # exception path of verify_kernel_packed
    e, per_len = 1, 200
    k, step = _index_of(min(MIXED_LENGTHS), e)
    rng = np.random.default_rng(4242)
    reads = [r for L in MIXED_LENGTHS for r in packed_reads(rng, world.seqs, world.places, per_len, L, e)]
    reads = [reads[int(j)] for j in rng.permutation(len(reads))]
    reads, kind = packed_exceptions(rng, reads, 0.03)
    assert np.any(kind == 1) and np.any(kind == 2)
    want = _oracle(world, reads, e, k, step)
    strand = np.repeat(np.arange(2 * len(reads)) & 1, np.diff(want.cand_off.astype(np.int64)))
    length = np.repeat(np.repeat([len(r) for r in reads], 2), np.diff(want.cand_off.astype(np.int64)))
    for L in MIXED_LENGTHS:
        ok = want.v_ed[length == L] != 255
        assert np.any(ok & (strand[length == L] == 0)) and np.any(ok & (strand[length == L] == 1)), L
        assert np.any(~ok), L
    bases = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    dev = world.dev(k, step, False)
    dev.stage_reads(bases, off)
    assert not dev.stage_info()[1]
    dev.map_staged(e=e, k=k, step=step)
    got = dev.fetch()
    off_g, cand, ed, end = got.per_strand()
    assert np.array_equal(off_g, want.cand_off) and np.array_equal(cand, want.cands)
    assert np.array_equal(ed, want.v_ed) and np.array_equal(end, want.v_end)
    assert len(got.stats) == 5 and np.array_equal(got.stats, want.stats)
