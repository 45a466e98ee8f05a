"""The BGZF compressor (fem_dev_bgzf_compress alone) at the edges its other tests do not reach: the 15-bit and 7-bit limits of
its code lengths, the far end of the 32768-byte window, members of 1 to 330 bytes and just under 65280, full HLIT and HDIST,
and members that must not see each other.  Every member is inflated by zlib (tests/harness.py: check_members) and read by
tests/deflate_model.py, which says what was written: block type, code lengths, tokens.  Needs a GPU: -m gpu."""
import zlib

import pytest

from tests import deflate_model as dm
from tests.harness import check_members

pytestmark = pytest.mark.gpu

DEEP = {"128x400+12": (1, 128, 400, 12), "64x700+13": (1, 64, 700, 13)}
FIB = {"3000": (3, 3000), "9000": (3, 9000)}


@pytest.fixture(scope="module")
def dev():
    from fem_amd import Device
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def inputs():
    """The larger inputs, made once."""
    out = {"deep " + k: dm.deep_literals(*a) for k, a in DEEP.items()}
    out.update({"fib " + k: dm.fib_runs(*a) for k, a in FIB.items()})
    out.update({"far %d" % g: dm.far_match(g) for g in (32767, 32768, 32769)})
    out["full"], out["zeros"] = dm.full_alphabets(), bytes(dm.MEMBER_INPUT)
    return out


def read_members(dev, data, level=1):
    """data through the compressor -> (its output, one deflate_model.Block per member).  Every member inflates with zlib to its
    part of data, has the right CRC-32, ISIZE and BSIZE and is no larger than its stored form (check_members); the reader gets
    the same bytes from a single block that ends where the CRC begins; and no token of any stream of this module has a length
    over 258, a distance over 32768 or one that reaches before the member's start."""
    out = dev.bgzf_compress(data, level)
    members, blocks, at = check_members(out, data), [], 0
    for raw, size, btype in members:
        read, end = dm.inflate(out, at + 18)
        assert len(read) == 1 and end == at + size - 8, "one final block that ends at the CRC"
        b = read[0]
        assert b.data == raw and b.btype == btype and b.btype in (0, 2)
        pos = 0
        for t in b.tokens:
            if isinstance(t, tuple):
                assert 3 <= t[0] <= dm.MAX_MATCH and 1 <= t[1] <= min(dm.WINDOW, pos), (t, pos)
                pos += t[0]
            else:
                pos += 1
        assert pos == len(raw)
        blocks.append(b)
        at += size
    return out, blocks


def matches(b):
    return [t for t in b.tokens if isinstance(t, tuple)]


def histogram(symbols, n):
    h = [0] * n
    for s in symbols:
        h[s] += 1
    return h


@pytest.mark.parametrize("which", list(DEEP))
def test_literal_code_limited_to_15_bits(dev, inputs, which):
    """No match is possible and the unlimited tree of the bytes is 19 deep, so the lengths come from the limiter: the longest
    is exactly 15, the code is complete (the reader), no symbol has a longer code than a rarer one, and the block is no larger
    than zlib's Huffman-only block of the same tokens plus 1 %.  Measured on the MI355X: 45 701 and 34 902 bytes, 0.9988 and
    0.9987 of zlib's size."""
    data = inputs["deep " + which]
    out, (b,) = read_members(dev, data)
    assert b.btype == 2 and not matches(b) and bytes(b.tokens) == data
    fl, _ = dm.token_histograms(b.tokens)
    assert dm.huffman_depth(fl) > 15, "the input no longer drives the tree past the limit"
    assert max(b.lit_lengths) == 15
    used = sorted((f, l) for f, l in zip(fl, b.lit_lengths) if f)
    assert all(l > 0 for _, l in used) and all(l == 0 for f, l in zip(fl, b.lit_lengths) if not f)
    for k, (f, l) in enumerate(used):  # every rarer symbol's code is at least as long
        assert all(l2 >= l for f2, l2 in used[:k] if f2 < f), (f, l)
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    ref = len(c.compress(data) + c.flush())
    print("deep_literals %s: %d bytes of deflate data, %.4f x zlib's Huffman-only block" % (which, len(out) - 26, (len(out) - 26) / ref))
    assert len(out) - 26 <= 1.01 * ref, (len(out) - 26, ref)


@pytest.mark.parametrize("which", list(FIB))
def test_code_length_code_limited_to_7_bits(dev, inputs, which):
    """The header's run-length symbols, as written, have an unlimited tree deeper than 7 (a condition on the input, read from
    the device's own stream), so the code-length alphabet's lengths come from the limiter: the longest is exactly 7 and the
    code is complete (the reader)."""
    out, (b,) = read_members(dev, inputs["fib " + which])
    assert b.btype == 2
    depth = dm.huffman_depth(histogram(b.cl_symbols, 19))
    print("fib_runs %s: %d code-length symbols, unlimited depth %d, longest code %d" % (which, len(b.cl_symbols), depth, max(b.cl_lengths)))
    assert depth > 7, "the input no longer drives the code-length alphabet past its limit"
    assert max(b.cl_lengths) == 7
    assert all((f > 0) == (l > 0) for f, l in zip(histogram(b.cl_symbols, 19), b.cl_lengths))


def test_window_edge(dev, inputs):
    """A 258-byte copy 32767 and 32768 bytes back is found; 32769 bytes back it is out of the window and costs 200 literals."""
    blocks = {g: read_members(dev, inputs["far %d" % g])[1][0] for g in (32767, 32768, 32769)}
    for g in (32767, 32768):
        assert blocks[g].btype == 2 and (258, g) in matches(blocks[g]), g
    assert max(d for _, d in matches(blocks[32769])) <= dm.WINDOW

    def literals(b):
        return len(b.tokens) - len(matches(b))
    assert literals(blocks[32769]) >= literals(blocks[32768]) + 200


def test_sizes(dev):
    """Every size from 1 to 330 and from 65216 to 65280, at levels 0 and 1, one call per member."""
    kinds = {}
    for content, n, data in dm.size_sweep():
        (b0,), (b,) = read_members(dev, data, 0)[1], read_members(dev, data, 1)[1]
        assert b0.btype == 0, (content, n)
        if n < 16:
            assert b.btype == 0, (content, n)
        kinds.setdefault(content, []).append((n, b, len(b.data) + 5 if b.btype == 0 else (b.bits + 7) // 8))
    for content in ("byte", "period2"):
        sizes = [x for x in kinds[content] if x[0] >= 16]
        dynamic = [k for k, (n, b, size) in enumerate(sizes) if b.btype == 2]
        assert dynamic, content
        # A member is stored only where its dynamic block would be no smaller.  That block is not seen, but the one of the next
        # size up that was written dynamic is: it has the same literals and one match that is longer, so at most one length
        # code, its extra bits and a run in the header differ, 3 bytes at the very most.
        for k, (n, b, size) in enumerate(sizes):
            if b.btype == 0:
                later = [j for j in dynamic if j > k]
                assert later and sizes[later[0]][2] + 3 >= n + 5, (content, n, "stored, though %d bytes are dynamic in %d"
                                                                   % (sizes[later[0]][0], sizes[later[0]][2]))
        assert all(b.btype == 2 for n, b, size in sizes[dynamic[0]:]), content  # dynamic from the first such size on
        for n, b, size in sizes[dynamic[0]:]:
            # the greedy parse ends on a match that stops exactly at n, unless 1 or 2 bytes are left over after matches of 258
            m = [k for k, t in enumerate(b.tokens) if isinstance(t, tuple)]
            lead, tail = m[0], len(b.tokens) - 1 - m[-1]
            assert lead == (1 if content == "byte" else 2), (content, n)
            assert tail == ((n - lead) % 258 if (n - lead) % 258 in (1, 2) else 0), (content, n, tail)
            assert all(t == (258, lead) for t in matches(b)[:-1]) and matches(b)[-1][1] == lead, (content, n)


def test_full_alphabets(dev, inputs):
    """HLIT = 286 with HDIST = 30 in one member that is kept: every literal, every length code and every distance code used."""
    (b,) = read_members(dev, inputs["full"])[1]
    assert b.btype == 2 and (b.hlit, b.hdist) == (286, 30)
    fl, fd = dm.token_histograms(b.tokens)
    assert all(fl) and all(fd), ([k for k, f in enumerate(fl) if not f], [k for k, f in enumerate(fd) if not f])
    assert all(b.lit_lengths) and all(b.dist_lengths)


@pytest.mark.parametrize("which,used", [("deep 128x400+12", 0), ("deep 64x700+13", 0), ("zeros", 1)])
def test_fewer_than_two_distances_used(dev, inputs, which, used):
    """No distance code used, or one: the block has two distance codes of one bit (a complete code), in a member that is kept."""
    (b,) = read_members(dev, inputs[which])[1]
    assert b.btype == 2 and b.dist_lengths == [1, 1]
    assert sum(1 for f in dm.token_histograms(b.tokens)[1] if f) == used


def test_members_do_not_see_each_other(dev, inputs):
    """Three members that reach the limiters and the window edge, filled up with random letters, and a short tail: compressed
    in one call they are, byte for byte, what separate calls give, and a second call gives the same bytes."""
    parts = [dm.padded(inputs[k], 11 + i) for i, k in enumerate(("deep 128x400+12", "fib 9000", "far 32768"))]
    parts.append(dm.padded(b"", 20)[:1000])
    whole = b"".join(parts)
    out, blocks = read_members(dev, whole)
    assert [len(b.data) for b in blocks] == [len(p) for p in parts]
    assert out == b"".join(dev.bgzf_compress(p, 1) for p in parts)
    assert dev.bgzf_compress(whole, 1) == out
    assert (258, 32768) in matches(blocks[2]) and all(b.btype == 2 for b in blocks)
