"""A batch mapped in parts (plan_parts, launch_batch, enqueue_packed in fem_amd/csrc/fem_hip.hip): a batch of 2 * 65536 reads or
more that meets an idle device with a dense index is cut at multiples of 64 reads; part q's selection runs on the side stream
as soon as its codes have arrived, its join on the slot's stream behind it.  That is the first batch of every job, and no
other test stages that many reads.

Every case stages its batch packed on a FRESH handle (nothing pending: the device is idle) under FEM_FORCE_DENSE=1 and
FEM_TIMELINE=1 and asserts
  - that the batch went in parts: the slot's timeline has `parts` selections (id 8) and `parts` joins (id 0) per launch of the
    batch, and one of each on the handle opened with FEM_NO_PARTS=1;
  - the per-strand arrays and the five counters of the whole batch equal those of that FEM_NO_PARTS handle;
  - the reads within 1000 of every part boundary and of both ends of the batch equal the oracle's, none left out.
The batches: n = 2 * 65536 + 77 reads of 100 bases, e = 3 — the smallest that splits in two; the boundary falls at read 65536
and the second part's size (65613) is a multiple of neither 64 nor 16 — and 4 * 65536 + 77 reads under FEM_PARTS=4.
Needs a GPU: -m gpu."""
import os
import re

import numpy as np
import pytest

from oracle import fem_oracle as fo
from tests.harness import device_with_env, library_stderr

pytestmark = pytest.mark.gpu

K, STEP, E, L = 12, 3, 3, 100
PART_MIN = 1 << 16  # kPartMinReads
N2, N4 = 2 * PART_MIN + 77, 4 * PART_MIN + 77
NEAR = 1000
ODD_READ = PART_MIN + 5  # the read that holds an N in the batch that is copied whole


def _cuts(n, parts):
    """plan_parts' rule: part q begins at (n q / parts) rounded down to a multiple of 64."""
    return [0] + [(n * q // parts) & ~63 for q in range(1, parts)] + [n]


def _spans(n, parts):
    spans = [(max(0, c - NEAR), min(n, c + NEAR)) for c in _cuts(n, parts)]
    assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))
    return spans


class _World:
    def __init__(self):
        from fem_amd import device, host
        text, off, lens = host.synth_reference(2028, [250_000, 90_000], threads=8)
        unit = text[1000:1400].copy()  # a unit of 400 bases at eight places: reads inside it have several candidates
        for at in range(30_000, 240_000, 30_000):
            text[at:at + 400] = unit
        self.seqs = [text[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(off, lens)]
        self.ref = fo.Reference(self.seqs)
        self.idx = fo.OracleIndex(self.ref, K, STEP)
        bases = host.synth_reads(28, text, off, lens, N4, L, E, threads=8)[0][:N4 * L]
        odd = bases[:N2 * L].copy()
        odd[ODD_READ * L + L // 2] = ord("N")
        self.bases = {"two": bases[:N2 * L], "odd": odd, "four": bases}
        self.packed, self.want, self.whole = {}, {}, {}
        for name, b in self.bases.items():
            n = len(b) // L
            buf = np.zeros(n * L + 64, np.uint8)
            self.packed[name] = (buf, device.pack_reads(b, n, L, buf))
        assert [self.packed[name][1] for name in ("two", "odd", "four")] == [0, 1, 0]
        self.plain = self.device(FEM_NO_PARTS="1")  # every batch mapped whole, once

    def device(self, **env):
        for name in ("FEM_NO_PARTS", "FEM_PARTS", "FEM_NO_OVERLAP", "FEM_TEST_TINY_BUFFERS", "FEM_FORCE_GENERIC", "FEM_NO_DENSE"):
            assert name in env or os.environ.get(name, "0") == "0", name
        dev = device_with_env(FEM_FORCE_DENSE="1", FEM_TIMELINE="1", **env)
        dev.upload_reference(self.seqs)
        dev.upload_index(K, STEP, self.idx.lookup, self.idx.occ[:self.idx.n_occ])
        assert dev.seed_kernel(e=E, k=K, step=STEP) == "seed_join_kernel"
        dev.set_timing(True)
        return dev

    def run(self, dev, name):
        """The batch staged packed, mapped and fetched -> (offsets, candidates, edit distances, ends, counters), and how many
        selections, joins and generic kernels slot 0's timeline shows."""
        buf, n_exc = self.packed[name]
        n = len(self.bases[name]) // L
        dev.reset_timing()
        with library_stderr() as err:
            hb, _ = dev.acquire_stage(n, n * L)
            hb[:len(buf)] = buf
            dev.commit_stage_packed(n, L, n_exc)
            assert dev.stage_info()[1]
            dev.map_staged(e=E, k=K, step=STEP)
            got = dev.fetch()
        assert dev.stage_front()[0]  # selected from the codes
        lines = re.findall(r"^TL slot 0 id +(\d+) ", err[0], re.M)
        return got.per_strand() + (got.stats,), tuple(lines.count(i) for i in ("8", "0", "2"))

    def mapped_whole(self, name):
        if name not in self.whole:
            self.whole[name], launches = self.run(self.plain, name)
            assert launches == (1, 1, 1), launches
        return self.whole[name]

    def oracle(self, name, parts):
        """The oracle's result of the reads near the cuts, as one batch."""
        if name not in self.want:
            b = self.bases[name]
            near = np.concatenate([b[lo * L:hi * L] for lo, hi in _spans(len(b) // L, parts)])
            batch = fo.ReadBatch.from_arrays(np.concatenate([near, np.zeros(8, np.uint8)]), np.arange(len(near) // L + 1, dtype=np.uint64) * L)
            self.want[name] = fo.map_reads(self.ref, self.idx, batch, e=E, k=K, step=STEP, threads=8, stages=fo.STAGE_SEED | fo.STAGE_VERIFY)
        return self.want[name]

    def close(self):
        self.plain.close()


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    w.close()


def _check(world, name, parts, reruns=False, **env):
    n = len(world.bases[name]) // L
    assert _cuts(N2, 2)[1] == PART_MIN and (N2 - PART_MIN) % 16 != 0
    dev = world.device(**env)
    try:
        got, (n_select, n_join, n_launch) = world.run(dev, name)
    finally:
        dev.close()
    print("parts %d: %d selections, %d joins, %d launches of the batch" % (parts, n_select, n_join, n_launch))
    assert (n_launch > 1) == reruns, n_launch
    assert (n_select, n_join) == (parts * n_launch, parts * n_launch)
    # the whole batch against the same batch mapped whole
    whole = world.mapped_whole(name)
    for g, w, what in zip(got, whole, ("candidate counts", "candidates", "edit distances", "end offsets", "counters")):
        assert np.array_equal(g, w), what
    assert len(got[4]) == 5 and int(got[4][0]) == n
    # the reads near the cuts against the oracle
    want = world.oracle(name, parts)
    off, cand, ed, end, _ = got
    spans = _spans(n, parts)
    assert sum(hi - lo for lo, hi in spans) == (want.cand_off.size - 1) // 2 == 2 * NEAR * parts
    at = [(int(off[2 * lo]), int(off[2 * hi])) for lo, hi in spans]
    counts = np.concatenate([np.diff(off[2 * lo:2 * hi + 1].astype(np.int64)) for lo, hi in spans])
    cand, ed, end = (np.concatenate([a[lo:hi] for lo, hi in at]) for a in (cand, ed, end))
    assert np.array_equal(counts, np.diff(want.cand_off.astype(np.int64))), "candidate counts per (read, strand)"
    assert np.array_equal(cand, want.cands), "candidate locations"
    assert np.array_equal(ed, want.v_ed), "edit distances / accept set"
    assert np.array_equal(end[ed != 0xFF], want.v_end[want.v_ed != 0xFF]), "end offsets"
    assert np.count_nonzero(want.v_ed != 0xFF) > NEAR and np.any(counts > 4)  # reads that map, some in the planted unit


def test_copied_in_parts_and_mapped_in_parts(world):
    _check(world, "two", 2)


def test_copied_whole_and_mapped_in_parts_behind_the_zeroing(world):
    """One read holds an N: the batch has an exception and is copied whole (enqueue_packed); launch_batch splits it."""
    _check(world, "odd", 2)


def test_the_rerun_after_an_overflow_splits_on_its_own(world):
    """Tiny scratch buffers: fem_dev_sync grows them and launches the batch again, not copied in parts this time."""
    _check(world, "two", 2, reruns=True, FEM_TEST_TINY_BUFFERS="1")


def test_four_parts(world):
    _check(world, "four", 4, FEM_PARTS="4")
