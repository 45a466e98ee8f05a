"""tests/deflate_model.py held to its own conditions, without a GPU: the reader against zlib's streams of every block type,
its refusal of bad code length sets, huffman_depth, and what each input generator promises the compressor's edge tests."""
import zlib

import numpy as np
import pytest

from tests import deflate_model as dm


def _deflate(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def _streams():
    rng = np.random.default_rng(21)
    text = b"".join(bytes(rng.integers(65, 69, int(n), dtype=np.uint8)) + b"\n" for n in rng.integers(1, 400, 600))
    return {"text": text, "deep": dm.deep_literals(1), "runs": dm.fib_runs(3, 9000) * 4, "far": dm.far_match(32768),
            "full": dm.full_alphabets(), "random": rng.bytes(200_000), "empty": b"", "one": b"x"}


@pytest.fixture(scope="module")
def streams():
    return _streams()


@pytest.mark.parametrize("level,strategy,btypes", [(1, zlib.Z_DEFAULT_STRATEGY, None), (9, zlib.Z_DEFAULT_STRATEGY, None),
                                                   (6, zlib.Z_FIXED, {0, 1}), (6, zlib.Z_HUFFMAN_ONLY, None), (0, zlib.Z_DEFAULT_STRATEGY, {0})])
def test_reader_reproduces_zlib_streams(streams, level, strategy, btypes):
    several = 0
    for name, data in streams.items():
        z = _deflate(data, level, strategy)
        blocks, end = dm.inflate(b"\xAA" * 3 + z + b"\x55" * 2, at=3)
        assert end == 3 + len(z), name
        assert b"".join(b.data for b in blocks) == data, name
        assert [b.final for b in blocks] == [0] * (len(blocks) - 1) + [1]
        several += len(blocks) > 1
        at = 0
        for b in blocks:
            assert b.first == at and (btypes is None or b.btype in btypes), name
            at += len(b.data)
            n = 0
            for t in b.tokens:  # the tokens are what the data says they are
                if isinstance(t, tuple):
                    assert 3 <= t[0] <= dm.MAX_MATCH and 1 <= t[1] <= min(dm.WINDOW, b.first + n), name
                    n += t[0]
                else:
                    n += 1
            assert n == len(b.data)
            if strategy == zlib.Z_HUFFMAN_ONLY:
                assert not any(isinstance(t, tuple) for t in b.tokens)
            if b.btype == 2:
                assert 257 <= b.hlit == len(b.lit_lengths) <= 286 and 1 <= b.hdist == len(b.dist_lengths) <= 30 and 4 <= b.hclen <= 19
                for lengths, top in ((b.cl_lengths, 7), (b.lit_lengths, 15), (b.dist_lengths, 15)):
                    assert max(lengths) <= top
                    assert sum(2.0 ** -l for l in lengths if l) == 1.0  # (zlib writes complete codes, of two codes at least)
                assert all(s <= 18 and b.cl_lengths[s] for s in b.cl_symbols) and len(b.cl_symbols) <= b.hlit + b.hdist
                fl, fd = dm.token_histograms(b.tokens)
                assert all((f > 0) <= (l > 0) for f, l in zip(fl, b.lit_lengths + [0] * 30)), name  # every symbol used has a code
                assert all((f > 0) <= (l > 0) for f, l in zip(fd, b.dist_lengths + [0] * 30)), name
    assert several >= 2  # several blocks per stream were seen


def _header(lit, dist):
    """A dynamic block's header with these lengths, each written as its own code-length symbol; the code-length alphabet gives
    4 bits to each of 0..15, so a symbol's code is its value.  -> (the bits as an int, their count)."""
    hlit, hdist = max(257, len(lit)), max(1, len(dist))
    lit, dist = list(lit) + [0] * (hlit - len(lit)), list(dist) + [0] * (hdist - len(dist))
    v = 1 | (2 << 1) | ((hlit - 257) << 3) | ((hdist - 1) << 8) | (15 << 13)
    pos = 17
    for s in dm.CL_ORDER:
        v |= (4 if s < 16 else 0) << pos
        pos += 3
    for l in lit + dist:
        v |= int(format(l, "04b")[::-1], 2) << pos  # (Huffman codes go in from their most significant bit)
        pos += 4
    return v, pos


def _stream(lit, dist, symbols=()):
    """The header of _header and then these (code, bits) pairs -> bytes."""
    v, pos = _header(lit, dist)
    for c, n in symbols:
        v |= c << pos
        pos += n
    return v.to_bytes((pos + 7) // 8 + 4, "little")


def test_reader_refuses_bad_code_lengths():
    # a complete code: 'a' and 'b' in 2 bits, end of block in 1
    lit = [0] * 257
    lit[97], lit[98], lit[256] = 2, 2, 1
    eob, a = (0, 1), (0b01, 2)  # canonical: 256 -> 0, 97 -> 10, 98 -> 11, written from the most significant bit
    blocks, _ = dm.inflate(_stream(lit, [1, 1], symbols=[a, a, eob]))
    assert blocks[0].data == b"aa" and blocks[0].btype == 2 and blocks[0].lit_lengths == lit and blocks[0].dist_lengths == [1, 1]
    assert blocks[0].cl_symbols == lit + [1, 1] and blocks[0].hclen == 19
    # deflate's exception: one distance code of one bit, or none, is no error
    assert dm.inflate(_stream(lit, [1], symbols=[a, eob]))[0][0].data == b"a"
    assert dm.inflate(_stream(lit, [0], symbols=[a, eob]))[0][0].data == b"a"
    over, under, two = list(lit), list(lit), list(lit)
    over[99] = 2
    under[98] = 3
    two[256] = 0
    for bad_lit, bad_dist, what in ((over, [1, 1], "over-subscribed"), (under, [1, 1], "incomplete"), (two, [1, 1], "end of the block"),
                                    (lit, [1, 1, 1], "over-subscribed"), (lit, [2, 2], "incomplete"), (lit, [2], "incomplete"),
                                    (lit, [0, 0, 3], "incomplete")):
        with pytest.raises(dm.DeflateError, match=what):
            dm.inflate(_stream(bad_lit, bad_dist, symbols=[a, eob]))
    # the code-length alphabet's own lengths
    for cl, what in (([4] * 16 + [4, 0, 0], "over-subscribed"), ([4] * 15 + [0] * 4, "incomplete")):
        v, pos = 1 | (2 << 1) | (15 << 13), 17
        for s in dm.CL_ORDER:
            v |= cl[s] << pos
            pos += 3
        with pytest.raises(dm.DeflateError, match="code-length alphabet: " + what):
            dm.inflate(v.to_bytes(16, "little"))
    # check_code itself
    with pytest.raises(dm.DeflateError):
        dm.check_code([1, 2, 3, 3, 3], "x")
    dm.check_code([1, 2, 3, 3], "x")
    with pytest.raises(dm.DeflateError, match="incomplete"):
        dm.check_code([1, 2, 3], "x")
    with pytest.raises(dm.DeflateError, match="incomplete"):
        dm.check_code([2], "x", single_ok=True)
    # a match that reaches before the start, a stored block whose NLEN is wrong, a stream that ends early
    ln3 = list(lit)
    ln3[97], ln3[98], ln3[256], = 2, 0, 2
    ln3 += [1]  # 257: length 3
    with pytest.raises(dm.DeflateError, match="distance of 2 after 1"):
        dm.inflate(_stream(ln3, [1, 1], symbols=[(0b01, 2), (0, 1), (1, 1), (0b11, 2)]))  # 'a', length 3, distance 2
    assert dm.inflate(_stream(ln3, [1, 1], symbols=[(0b01, 2), (0, 1), (0, 1), (0b11, 2)]))[0][0].tokens == [97, (3, 1)]
    with pytest.raises(dm.DeflateError, match="NLEN"):
        dm.inflate(b"\x01\x02\x00\xfd\xfe..")
    z = _deflate(b"abcabcabc" * 50, 6)
    with pytest.raises(dm.DeflateError, match="ends inside"):
        dm.inflate(z[:-2])


def test_huffman_depth():
    assert dm.huffman_depth([]) == 0 and dm.huffman_depth([0, 7, 0]) == 1 and dm.huffman_depth([1, 1]) == 1
    assert dm.huffman_depth([1] * 8) == 3 and dm.huffman_depth([1] * 9) == 4
    assert dm.huffman_depth([1, 1, 2, 3, 5, 8, 13, 21]) == 7  # Fibonacci weights: a chain
    assert dm.huffman_depth([1, 1, 1, 1, 2, 2]) == 3  # ties go to the shallower subtree: 3, where the other choice gives 4
    # against the lengths zlib gives where its limit of 15 is far away: both are optimal, and zlib breaks ties the same way
    rng = np.random.default_rng(4)
    for _ in range(20):
        f = [int(x) for x in rng.integers(1, 1000, int(rng.integers(2, 200)))]
        data = b"".join(bytes([s]) * c for s, c in enumerate(f))
        data = bytes(rng.permutation(np.frombuffer(data, np.uint8)))
        b = dm.inflate(_deflate(data, 6, zlib.Z_HUFFMAN_ONLY))[0][0]
        fl = dm.token_histograms(b.tokens)[0]
        cost = sum(c * l for c, l in zip(fl, b.lit_lengths))
        assert max(b.lit_lengths) >= dm.huffman_depth(fl) and cost == _optimal_cost(fl)


def _optimal_cost(freqs):
    """Bits of a Huffman code: the sum of the merged weights."""
    import heapq
    h = [f for f in freqs if f]
    heapq.heapify(h)
    total = 0
    while len(h) > 1:
        a = heapq.heappop(h) + heapq.heappop(h)
        total += a
        heapq.heappush(h, a)
    return total


@pytest.mark.parametrize("args,size", [((1,), 51808), ((1, 64, 700, 13), 45785), ((2,), 51808), ((3,), 51808),
                                       ((2, 64, 700, 13), 45785)])
def test_deep_literals(args, size):
    assert dm.rare_counts(12) == [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233]
    data = dm.deep_literals(*args)
    assert len(data) == size and data == dm.deep_literals(*args)
    R, W, m = (args + (128, 400, 12))[1:4] if len(args) > 1 else (128, 400, 12)
    counts = sorted(np.bincount(np.frombuffer(data, np.uint8), minlength=256))
    assert counts == [0] * (256 - R - m) + dm.rare_counts(m) + [W] * R
    a = np.frombuffer(data, np.uint8).astype(np.int64)
    tri = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
    assert len(np.unique(tri)) == len(tri)  # no three consecutive bytes occur twice
    fl, fd = dm.token_histograms(list(data))
    assert dm.huffman_depth(fl) >= 17 and not any(fd)
    # and zlib's own matcher finds nothing either: its level 9 stream has no match
    assert not any(isinstance(t, tuple) for b in dm.inflate(_deflate(data, 9))[0] for t in b.tokens)


def test_fib_runs_and_far_match_and_sweep():
    for seed, N, lo, hi in ((3, 3000, 16_000, 18_000), (3, 9000, 48_000, 53_000), (4, 3000, 16_000, 18_000), (4, 9000, 48_000, 53_000)):
        data = dm.fib_runs(seed, N)
        assert lo < len(data) < hi and data == dm.fib_runs(seed, N) and data != dm.fib_runs(seed + 10, N)
    assert len(dm.fib_runs(3, 20_000)) == dm.MEMBER_INPUT
    X = dm.FAR_ANCHOR
    assert len(X) == 200 == len(set(X)) and 0 not in X
    for gap in (32767, 32768, 32769):
        data = dm.far_match(gap)
        assert data[:200] == X and data[gap:gap + 200] == X and not any(data[200:gap]) and data[gap + 200:] == bytes(100)
        assert len(data) == gap + 300 <= dm.MEMBER_INPUT
    sweep = dm.size_sweep()
    assert [(c, n) for c, n, _ in sweep] == [(c, n) for c, n, _ in dm.size_sweep()] and all(a[2] == b[2] for a, b in zip(sweep, dm.size_sweep()))
    for content in dm.SWEEP_CONTENTS:
        sizes = [n for c, n, d in sweep if c == content]
        assert sizes[:329] == list(range(2, 331)) and all(len(d) == n for c, n, d in sweep)
        assert (sizes[329:] == list(range(65216, 65279))) == (content != "letters")
    assert all(d == d[:1] * n for c, n, d in sweep if c == "byte") and all(d == (d[:2] * n)[:n] for c, n, d in sweep if c == "period2")
    assert all(set(d) <= set(b"ABCD") for c, n, d in sweep if c == "letters")
    pad = dm.padded(b"xyz", 5)
    assert len(pad) == dm.MEMBER_INPUT and pad == dm.padded(b"xyz", 5) and pad != dm.padded(b"xyz", 6) and set(pad[3:]) == set(b"ABCD")


def test_full_alphabets_has_a_copy_for_every_code():
    data = dm.full_alphabets()
    assert data == dm.full_alphabets() and len(data) <= dm.MEMBER_INPUT and set(data) == set(range(256))
    # zlib at level 9 (an exhaustive matcher by comparison) uses the longest length and the farthest distance code on it
    fl, fd = [0] * 286, [0] * 30
    for b in dm.inflate(_deflate(data, 9))[0]:
        l, d = dm.token_histograms(b.tokens)
        fl, fd = [x + y for x, y in zip(fl, l)], [x + y for x, y in zip(fd, d)]
    assert fl[285] and fd[29] and all(fl[:256])
