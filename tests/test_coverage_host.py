"""fem_coverage_layout and fem_coverage_write of libfemhost.so: the windows' arithmetic with its cap and the BED text, byte for
byte.  No GPU."""
import numpy as np

from fem_amd import host
from tests import coverage_model as m


def test_layout_of_1_w_and_w_plus_1_bases():
    for W in (1, 7, 64, 1000):
        lens = [1, W, W + 1]
        rc, n_bins, off = host.coverage_layout(lens, W)
        want = [0, 1, 2, 4]  # 1, 1 and 2 windows
        assert rc == 0 and n_bins == 4 and off.tolist() == want == m.layout(lens, W)
    rc, n_bins, off = host.coverage_layout([200_000, 50_017], 1000)
    assert (rc, n_bins, off.tolist()) == (0, 251, [0, 200, 251])


def test_window_range():
    assert host.coverage_layout([100], 0)[0] == -1
    assert host.coverage_layout([100], 1_000_001)[0] == -1
    assert host.coverage_layout([100], 1_000_000)[:2] == (0, 1)
    assert host.coverage_layout([], 1000)[:2] == (0, 0)


def test_the_cap_is_arithmetic():
    # one sequence of 4 000 000 000 bases: 4e9 windows at W = 1, 5e8 <= 2^29 at W = 8; nothing of that size is allocated
    lens = [4_000_000_000]
    rc, n_bins, _ = host.coverage_layout(lens, 1)
    assert (rc, n_bins) == (-2, 4_000_000_000)
    rc, n_bins, off = host.coverage_layout(lens, 8)
    assert (rc, n_bins, off.tolist()) == (0, 500_000_000, [0, 500_000_000])
    assert host.coverage_layout(lens, 7)[0] == -2  # 571 428 572 > 2^29 = 536 870 912
    assert host.coverage_min_window(lens) == 8
    assert host.coverage_min_window([100, 200]) == 1
    # exactly 2^29 windows fit, one more does not
    assert host.coverage_layout([1 << 29], 1)[:2] == (0, 1 << 29)
    assert host.coverage_layout([1 << 29, 1], 1)[:2] == (-2, (1 << 29) + 1)
    assert host.coverage_min_window([1 << 29, 1]) == 2


def test_write_byte_for_byte(tmp_path):
    names, lens, W = ["chr_a", "b", "c"], [1, 8, 19], 8
    #        chr_a  b: h = (1 * 100 + 4) / 8 = 13  c: 10.00, 12.38 (99 / 8 = 12.375 -> h = 1238), last window of 3 bases: 7 / 3 -> 2.33
    track = [1, 1, 80, 99, 7]
    path = tmp_path / "cov.bed"
    total = host.coverage_write(str(path), names, lens, W, track)
    want = (b"chr_a\t0\t1\t1\t1.00\n" b"b\t0\t8\t1\t0.13\n" b"c\t0\t8\t80\t10.00\n" b"c\t8\t16\t99\t12.38\n" b"c\t16\t19\t7\t2.33\n")
    assert path.read_bytes() == want == m.bed(names, lens, W, np.array(track, np.uint64))
    assert total == sum(track)


def test_write_many_windows_and_large_counts(tmp_path):
    rng = np.random.default_rng(5)
    names, lens, W = ["s%d" % i for i in range(3)], [70_001, 3, 12_345], 7
    n = host.coverage_layout(lens, W)[1]
    track = rng.integers(0, 1 << 40, n).astype(np.uint64)
    track[:5] = [0, 1, 3, 4, (1 << 63) // 100]  # (bases * 100 stays inside 64 bits up to 2^64 / 100)
    path = tmp_path / "big.bed"
    total = host.coverage_write(str(path), names, lens, W, track)
    assert path.read_bytes() == m.bed(names, lens, W, track)  # (more text than one buffer of the writer holds)
    assert total == int(track.sum(dtype=np.uint64))
