"""seed_select_kernel's packed front end (fem_amd/csrc/fem_seed_select.hip.h) and characters on demand (ensure_chars,
fem_amd/csrc/fem_hip.hip): a batch that came packed — equal-length reads at two bits per base — has its seeds selected
straight from its codes on a dense index, and its characters are made only when something asks for them: the sparse seed
kernel, the device tail.  Every batch here is staged packed (pack_reads -> commit_stage_packed) under FEM_FORCE_DENSE=1 and
compared array for array, counters included, with the oracle and with a second handle on which FEM_SELECT_CHARS=1 keeps
the expansion at commit and the character front end.

Before anything runs on the GPU every case asserts, from its lengths and the index, that the selection keeps every read
(a >= 1, at most 128 DP columns, no bucket at the 16-bit limit): the packed front end, not the generic kernel, made the
seeds.  The banked selection is the same kernel body and gets the front end too (one case).
Needs a GPU: -m gpu."""
import os

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests import util
from tests.cases import packed_exceptions, packed_reads, packed_reference
from tests.harness import device_with_env

pytestmark = pytest.mark.gpu

K, STEP, A = 12, 3, 1
HALF = 200  # the planted palindrome x + revcomp(x): every read inside it maps on both strands
# (L, e): L mod 4 = 0, 1, 2, 3 around the stream's word boundaries, each with one e of {2, 3, 4, 7}, 13 + 12 (e + 2) <= L
CASES = [(100, 3), (101, 2), (102, 4), (103, 3), (111, 4), (112, 2), (113, 3), (127, 7), (128, 4), (129, 7), (150, 7),
         (301, 7)]
SIZES = (1, 6, 7, 8, 15, 16, 17, 257)  # sub-blocks of 7 (L = 103) or 8 (L = 100) reads, blocks of 16
N_READS = 600


class _World:
    def __init__(self):
        rng = np.random.default_rng(20261019)
        self.seqs, self.places = packed_reference(rng)
        x = util.rand_seq(rng, HALF)
        self.pal_at = len(self.seqs[3]) + 500
        self.seqs[3] = self.seqs[3] + util.rand_seq(rng, 500) + x + util.revcomp(x) + util.rand_seq(rng, 500)
        assert len(self.seqs) == 4 and sum(len(s) for s in self.seqs) < 400_000
        self.ref = fo.Reference(self.seqs)
        self.idx = fo.OracleIndex(self.ref, K, STEP)
        self.devs = {}

    def dev(self, chars=False, dense=True, banked=False):
        """A handle with the index; chars: under FEM_SELECT_CHARS=1; dense: FEM_FORCE_DENSE=1; banked: two banks of two."""
        key = (chars, dense, banked)
        if key not in self.devs:
            switches = {"FEM_SELECT_CHARS": chars, "FEM_FORCE_DENSE": dense, "FEM_TEST_BANK_SEQS": banked}
            for name in switches:
                assert os.environ.get(name, "0") == "0", name
            d = device_with_env(**{name: "2" if name == "FEM_TEST_BANK_SEQS" else "1" for name, on in switches.items() if on})
            d.upload_reference(self.seqs)
            d.upload_index(K, STEP, self.idx.lookup, self.idx.occ[:self.idx.n_occ])
            self.devs[key] = d
        return self.devs[key]

    def reads(self, rng, n, L, e):
        """Read 0 from inside the palindrome (accepted on both strands, whatever n), the rest from tests.cases.packed_reads."""
        at = self.pal_at + HALF - L // 2 if L <= 2 * HALF else self.pal_at
        first = self.seqs[3][at:at + L]
        return [first] + (packed_reads(rng, self.seqs, self.places, n - 1, L, e) if n > 1 else [])

    def close(self):
        for d in self.devs.values():
            d.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _assert_selection_keeps(world, L, e):
    """The shapes seed_select_kernel hands to the generic kernel (kSlow): a = 0, a phase group of more than 128 DP columns,
    a bucket of 65 535 entries or more.  None of them here: asserted from the length and the index, before the GPU runs."""
    R = e + 1 + A
    assert A >= 1
    assert 13 + 12 * (e + 2) <= L
    assert (L - K + 1) // STEP - R * 4 + 1 <= 128
    assert int(np.max(np.diff(world.idx.lookup.astype(np.int64)))) < 0xFFFF


def _oracle(world, reads, e):
    return fo.map_reads(world.ref, world.idx, fo.ReadBatch(reads), e=e, k=K, step=STEP, stages=fo.STAGE_SEED | fo.STAGE_VERIFY)


def _assert_both_strands(want, n):
    strand = np.repeat(np.arange(2 * n) & 1, np.diff(want.cand_off.astype(np.int64)))
    ok = want.v_ed != 255
    assert np.any(ok & (strand == 0)) and np.any(ok & (strand == 1)), "accepted candidates on both strands"


def _stage_packed(dev, reads, L):
    from fem_amd import device
    n = len(reads)
    bases = np.frombuffer(b"".join(reads), np.uint8)
    hb, _ = dev.acquire_stage(n, n * L)
    n_exc = device.pack_reads(bases, n, L, hb)
    assert n_exc == sum(sum(1 for c in r if c not in b"ACGT") for r in reads)
    dev.commit_stage_packed(n, L, n_exc)
    assert dev.stage_info()[1]
    return n_exc


def _run_packed(dev, reads, L, e, from_codes):
    n_exc = _stage_packed(dev, reads, L)
    if from_codes is not None:
        # characters at commit only under FEM_SELECT_CHARS=1 or above one exception per eight reads (kExpandAllShare)
        assert dev.stage_front()[1] == ((not from_codes) or n_exc * 8 > len(reads))
    dev.map_staged(e=e, a=A, k=K, step=STEP)
    got = dev.fetch()
    if from_codes is not None:
        assert dev.stage_front()[0] == from_codes  # which front end the batch took
    return got.per_strand() + (got.stats,)


def _check(world, reads, L, e, want=None, banked=False):
    _assert_selection_keeps(world, L, e)
    want = want or _oracle(world, reads, e)
    _assert_both_strands(want, len(reads))
    off, cand, ed, end, stats = _run_packed(world.dev(False, True, banked), reads, L, e, True)
    assert np.array_equal(off, want.cand_off) and np.array_equal(cand, want.cands)
    assert np.array_equal(ed, want.v_ed)
    assert np.array_equal(end[ed != 255], want.v_end[want.v_ed != 255])
    off_c, cand_c, ed_c, end_c, stats_c = _run_packed(world.dev(True, True, banked), reads, L, e, False)
    assert np.array_equal(off, off_c) and np.array_equal(cand, cand_c)
    assert np.array_equal(ed, ed_c) and np.array_equal(end, end_c)
    assert np.array_equal(stats, stats_c) and len(stats) == 5
    assert np.array_equal(stats, want.stats)


def _some_exceptions(rng, reads, share=0.03):
    """About 3 % of the reads with N, n, a lower-case base or R at the first, a middle and the last base; a small batch gets
    one such read at least."""
    odd, kind = packed_exceptions(rng, reads, share)
    if not np.any(kind) and len(reads) > 1:
        i = int(rng.integers(1, len(reads)))
        odd[i:i + 1] = packed_exceptions(rng, reads[i:i + 1], 1.0)[0]
    return odd


def _one_exception(reads, i, at, ch):
    """Read i with the single character ch at base `at`: one exception in the batch — from eight reads on that is below the
    share at which the batch is expanded whole (n_exc * 8 > n), so unpack_marked_reads_kernel alone makes its characters."""
    out = list(reads)
    r = bytearray(out[i])
    r[at] = ch if ch else r[at] | 0x20
    out[i] = bytes(r)
    return out


@pytest.mark.parametrize("L,e", CASES)
def test_every_length_against_the_oracle_and_the_character_front_end(world, L, e):
    rng = np.random.default_rng(1000 * L + e)
    reads = world.reads(rng, N_READS, L, e)
    _check(world, reads, L, e)
    _check(world, _some_exceptions(rng, reads), L, e)


@pytest.mark.parametrize("L", (100, 103))
@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_around_sub_blocks_and_blocks(world, L, n):
    e = 3
    rng = np.random.default_rng(77 * L + n)
    reads = world.reads(rng, n, L, e)
    _check(world, reads, L, e)
    if n > 1:
        _check(world, _some_exceptions(rng, reads), L, e)
    # the LAST read alone marked, by one character (N, R or a lower-case base by turns; first, middle or last base).  The
    # sub-blocks hold 7 reads at L = 103 and 8 at L = 100 (make_layout_select): a marked sub-block of one read at n = 1, 17 (a
    # block of its own) and, at L = 103, 8 and 15; of two reads at n = 16 there.  From n = 8 on the batch is below the share and
    # only that read is expanded at commit
    odd = _one_exception(reads, n - 1, (0, L // 2, L - 1)[n % 3], (ord("N"), ord("R"), 0)[(n // 3) % 3])
    _check(world, odd, L, e)


def test_a_batch_in_which_every_read_is_marked(world):
    L, e = 103, 3
    rng = np.random.default_rng(5)
    odd, kind = packed_exceptions(rng, world.reads(rng, 500, L, e), 1.0)
    assert np.all(kind > 0) and np.any(kind == 1) and np.any(kind == 2)
    _check(world, odd, L, e)


def test_only_the_first_and_the_last_read_marked(world):
    L, e = 101, 2
    rng = np.random.default_rng(6)
    reads = world.reads(rng, 500, L, e)
    for i in (0, len(reads) - 1):
        r = bytearray(reads[i])
        r[0], r[L // 2], r[L - 1] = r[0] | 0x20, ord("N"), r[L - 1] | 0x20
        reads[i] = bytes(r)
    _check(world, reads, L, e)


def test_the_banked_selection_reads_the_codes_too(world):
    L, e = 103, 3
    rng = np.random.default_rng(7)
    reads = world.reads(rng, 500, L, e)
    assert world.dev(False, True, True).seed_kernel(e=e) == "seed_join_banked_kernel"
    _check(world, reads, L, e, banked=True)
    _check(world, _some_exceptions(rng, reads), L, e, banked=True)


def _records(dev):
    r = dev.fetch_records()
    return (r.rec_begin, r.flag, r.tid, r.pos0, r.nm, r.cigar_off, r.cigar, r.md_off, r.md, r.stats)


def test_characters_on_demand_for_the_device_tail(world):
    L, e = 101, 3
    rng = np.random.default_rng(8)
    reads = _some_exceptions(rng, world.reads(rng, N_READS, L, e))
    _assert_selection_keeps(world, L, e)
    dev = world.dev(False, True)
    _stage_packed(dev, reads, L)
    dev.map_staged(e=e, a=A, k=K, step=STEP)
    dev.sync()
    assert dev.stage_front() == (True, False)  # mapped from the codes; nobody has asked for the characters
    first = _records(dev)
    assert dev.stage_front() == (True, True)   # the tail did
    again = _records(dev)                       # ... and the second fetch finds them (chars_ready)
    assert dev.stage_front() == (True, True)
    # the same batch staged as characters
    bases = np.frombuffer(b"".join(reads), np.uint8)
    hb, _ = dev.acquire_stage(len(reads), len(bases))
    hb[:len(bases)] = bases
    dev.commit_stage(len(reads), L, uniform=True)
    assert not dev.stage_info()[1]
    dev.map_staged(e=e, a=A, k=K, step=STEP)
    want = _records(dev)
    assert dev.stage_front() == (False, True)
    assert len(want[1]) > 0 and np.any(want[4] > 0)
    for g, a2, w in zip(first, again, want):
        assert np.array_equal(g, w) and np.array_equal(a2, w)


def test_sparse_index_expands_in_front_of_the_fast_seed_kernel(world):
    L, e = 103, 3
    rng = np.random.default_rng(9)
    reads = _some_exceptions(rng, world.reads(rng, N_READS, L, e))
    want = _oracle(world, reads, e)
    _assert_both_strands(want, len(reads))
    dev = world.dev(False, False)
    assert dev.seed_kernel(e=e).startswith("seed_fast_kernel")
    _stage_packed(dev, reads, L)
    assert not dev.stage_front()[1]
    off, cand, ed, end, stats = _run_packed(dev, reads, L, e, None)
    assert dev.stage_front() == (False, True)  # expanded on demand, selected from characters
    assert np.array_equal(off, want.cand_off) and np.array_equal(cand, want.cands)
    assert np.array_equal(ed, want.v_ed) and np.array_equal(end[ed != 255], want.v_end[want.v_ed != 255])
    assert np.array_equal(stats, want.stats)
