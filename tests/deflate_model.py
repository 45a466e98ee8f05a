"""A reader of raw deflate streams that reports what was written, and the inputs that drive the BGZF compressor to its edges.

The reader is made from RFC 1951 alone (struct, no zlib): per block it gives BTYPE, HLIT, HDIST, HCLEN, the code lengths of
the three alphabets, the code-length symbols as written, the tokens and the bytes they reproduce, and it refuses code length
sets that are over-subscribed or incomplete.  It knows nothing of how the device's compressor finds matches or builds codes:
the tests hold the stream it wrote to properties that any correct deflate encoder with those limits has.  The generators are
here so that the CPU test of their conditions and the GPU test share them; no test module imports another."""
import heapq
import struct

import numpy as np

MEMBER_INPUT = 65280  # bytes of input per BGZF member
WINDOW = 32768
MAX_MATCH = 258

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)  # RFC 1951 §3.2.7
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class DeflateError(ValueError):
    pass


class Block:
    """One deflate block as written.  For BTYPE 2: hlit, hdist, hclen (the counts, not the header fields: 257.., 1.., 4..),
    cl_lengths (19, by symbol), cl_symbols (the code-length symbols 0..18 in stream order), lit_lengths (hlit) and
    dist_lengths (hdist).  BTYPE 1 has the fixed lit_lengths and dist_lengths, BTYPE 0 has none.  tokens holds a literal as an
    int and a match as (length, distance); data is what the tokens reproduce; first is the offset of data in the stream's
    output and bits the size of the block in bits (a stored block's padding included)."""
    __slots__ = ("btype", "final", "hlit", "hdist", "hclen", "cl_lengths", "cl_symbols", "lit_lengths", "dist_lengths", "tokens",
                 "data", "first", "bits")

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, None)


class _Bits:
    def __init__(self, data, at):
        self.d, self.pos, self.end = bytes(data) + b"\0\0\0\0", 8 * at, 8 * len(data)

    def peek(self, n):  # n <= 24; bits past the end read as zero and are caught by take
        p = self.pos
        return (struct.unpack_from("<I", self.d, p >> 3)[0] >> (p & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.pos += n
        if self.pos > self.end:
            raise DeflateError("the stream ends inside a block")
        return v


def check_code(lengths, what, single_ok=False):
    """Refuse a set of code lengths that does not fill the code space exactly: over-subscribed or incomplete.  With
    single_ok (the distance alphabet, RFC 1951 §3.2.7) one code of one bit, or no code at all, passes as well."""
    used = [l for l in lengths if l]
    if single_ok and (not used or used == [1]):
        return
    if not used:
        raise DeflateError("%s: no code at all" % what)
    top = max(used)
    kraft = sum(1 << (top - l) for l in used)
    if kraft > 1 << top:
        raise DeflateError("%s: over-subscribed code lengths" % what)
    if kraft < 1 << top:
        raise DeflateError("%s: incomplete code lengths" % what)


def _decoder(lengths):
    """Canonical code of these lengths (RFC 1951 §3.2.2) -> (table over the next `top` bits as they lie in the stream, top).
    An entry is (symbol, length), or None where an incomplete code has no codeword."""
    top = max(lengths) if lengths else 0
    if top == 0:
        return [], 0
    count = [0] * (top + 1)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (top + 1), 0
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = [None] * (1 << top)
    for s, l in enumerate(lengths):
        if l:
            c, nxt[l] = nxt[l], nxt[l] + 1
            r = int(format(c, "0%db" % l)[::-1], 2)  # Huffman codes are packed from their most significant bit
            for k in range(r, 1 << top, 1 << l):
                table[k] = (s, l)
    return table, top


def _symbol(bits, dec, what):
    table, top = dec
    if not top:
        raise DeflateError("%s: a symbol of an alphabet without codes" % what)
    e = table[bits.peek(top)]
    if e is None:
        raise DeflateError("%s: bits that are no codeword" % what)
    bits.take(e[1])
    return e[0]


_FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_DIST = [5] * 32


def inflate(data, at=0):
    """Read the raw deflate stream that starts at byte `at` of data -> (blocks, the offset of the first byte after it)."""
    bits, out, blocks = _Bits(data, at), bytearray(), []
    while True:
        b, start = Block(), bits.pos
        b.final, b.btype, b.first = bits.take(1), bits.take(2), len(out)
        if b.btype == 3:
            raise DeflateError("BTYPE 3")
        if b.btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            if n ^ nn != 0xFFFF:
                raise DeflateError("stored block: LEN and NLEN disagree")
            p = bits.pos >> 3
            if p + n > bits.end >> 3:
                raise DeflateError("the stream ends inside a stored block")
            out += bits.d[p:p + n]
            bits.pos += 8 * n
            b.tokens = list(bits.d[p:p + n])
        else:
            if b.btype == 1:
                b.lit_lengths, b.dist_lengths = list(_FIXED_LIT), list(_FIXED_DIST)
            else:
                _dynamic_header(bits, b)
            _tokens(bits, b, _decoder(b.lit_lengths), _decoder(b.dist_lengths), out)
        b.data, b.bits = bytes(out[b.first:]), bits.pos - start
        blocks.append(b)
        if b.final:
            return blocks, (bits.pos + 7) >> 3


def _dynamic_header(bits, b):
    b.hlit, b.hdist, b.hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if b.hlit > 286 or b.hdist > 30:
        raise DeflateError("HLIT %d / HDIST %d" % (b.hlit, b.hdist))
    b.cl_lengths = [0] * 19
    for k in range(b.hclen):
        b.cl_lengths[CL_ORDER[k]] = bits.take(3)
    check_code(b.cl_lengths, "code-length alphabet")
    dec, lens, b.cl_symbols = _decoder(b.cl_lengths), [], []
    while len(lens) < b.hlit + b.hdist:
        s = _symbol(bits, dec, "code-length alphabet")
        b.cl_symbols.append(s)
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                raise DeflateError("code 16 with no length before it")
            lens += [lens[-1]] * (3 + bits.take(2))
        else:
            lens += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
    if len(lens) > b.hlit + b.hdist:
        raise DeflateError("a run of code lengths passes HLIT + HDIST")
    b.lit_lengths, b.dist_lengths = lens[:b.hlit], lens[b.hlit:]
    if not b.lit_lengths[256]:
        raise DeflateError("no code for the end of the block")
    check_code(b.lit_lengths, "literal/length alphabet")
    check_code(b.dist_lengths, "distance alphabet", single_ok=True)


def _tokens(bits, b, lit, dist, out):
    b.tokens = []
    while True:
        s = _symbol(bits, lit, "literal/length alphabet")
        if s < 256:
            out.append(s)
            b.tokens.append(s)
        elif s == 256:
            return
        else:
            if s > 285:
                raise DeflateError("length symbol %d" % s)
            length = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
            d = _symbol(bits, dist, "distance alphabet")
            if d > 29:
                raise DeflateError("distance symbol %d" % d)
            distance = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
            if distance > len(out):
                raise DeflateError("a distance of %d after %d bytes" % (distance, len(out)))
            for _ in range(length):  # (byte by byte: a match may overlap itself)
                out.append(out[-distance])
            b.tokens.append((length, distance))


def length_symbol(length):
    return 257 + max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 285


def distance_symbol(distance):
    return max(k for k in range(30) if DIST_BASE[k] <= distance)


def token_histograms(tokens):
    """-> (286 literal/length counts with one end-of-block, 30 distance counts) of a block's tokens."""
    fl, fd = [0] * 286, [0] * 30
    fl[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            fl[length_symbol(t[0])] += 1
            fd[distance_symbol(t[1])] += 1
        else:
            fl[t] += 1
    return fl, fd


def huffman_depth(freqs):
    """The deepest leaf of an unlimited Huffman tree over the non-zero entries of freqs, built with a heap of
    (weight, height, serial).  Of equal weights the subtree of the smaller height is merged first, then the older one: the
    rule that keeps a Huffman tree as shallow as its weights allow, so a depth reported here is one that no choice among ties
    avoids.  One symbol alone has depth 1 (it still needs a bit), none has depth 0."""
    heap = [(f, 0, k) for k, f in enumerate(f for f in freqs if f)]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    serial = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, serial))
        serial += 1
    return heap[0][1]


# ---- inputs ----

def rare_counts(m):
    """s_1 = 1, s_(i+1) = max(s_i, acc_(i-1)) + 1 with acc_0 = 1 for the end-of-block symbol: 1, 2, 3, 5, 8, 13, 21, ...  Every
    count exceeds the sum of all counts two places below it, so each joins the Huffman tree one level above the last, and the
    strict growth leaves no tie that could flatten it."""
    s, acc = [1], [1, 2]
    while len(s) < m:
        s.append(max(s[-1], acc[-2]) + 1)
        acc.append(acc[-1] + s[-1])
    return s


def deep_literals(seed, R=128, W=400, m=12):
    """R byte values W times each and m rare ones with rare_counts(m), in an order in which no three consecutive bytes occur
    twice: no LZ77 matcher finds a match, the tokens are the bytes, and their unlimited Huffman tree is deeper than 15."""
    rng = np.random.default_rng(seed)
    values = [int(v) for v in rng.permutation(256)[:R + m]]
    pool = []
    for v in values[:R]:
        pool += [v] * W
    for v, s in zip(values[R:], rare_counts(m)):
        pool += [v] * s
    pool = [pool[i] for i in rng.permutation(len(pool))]
    out, seen = bytearray(), set()
    while pool:
        j = len(pool) - 1
        if len(out) >= 2:
            head = (out[-2] << 16) | (out[-1] << 8)
            while j >= 0 and (head | pool[j]) in seen:
                j -= 1
            if j < 0:
                raise ValueError("deep_literals(%d, %d, %d, %d): every byte left completes a sequence already emitted"
                                 % (seed, R, W, m))
            seen.add(head | pool[j])
        out.append(pool.pop(j))
    return bytes(out)


def fib_runs(seed, N):
    """N runs of one byte value each (uniform over 256), of 4 + j bytes with P(j) ~ phi^-j over 24 values of j, cut at one
    member's input.  The code lengths of such a member's block come in runs whose counts fall off like Fibonacci numbers,
    which is what drives the code-length alphabet's tree past 7 levels."""
    rng = np.random.default_rng(seed)
    p = ((1 + 5 ** 0.5) / 2) ** -np.arange(24.0)
    values, js = rng.integers(0, 256, N), rng.choice(24, N, p=p / p.sum())
    return b"".join(bytes([int(v)]) * (4 + int(j)) for v, j in zip(values, js))[:MEMBER_INPUT]


FAR_ANCHOR = bytes(range(1, 201))  # 200 distinct non-zero bytes


def far_match(gap):
    """The anchor, zeros up to offset gap, the anchor again, 100 zeros.  The zeros repeat one 3-byte sequence only, so
    whatever a matcher remembers of the anchor's first copy is still there when the second arrives, `gap` bytes on."""
    return FAR_ANCHOR + bytes(gap - len(FAR_ANCHOR)) + FAR_ANCHOR + bytes(100)


SWEEP_HELD_ELSEWHERE = (1, 65279, 65280)  # sizes that the compressor's older test already feeds it
SWEEP_CONTENTS = ("byte", "period2", "letters")


def size_sweep():
    """-> [(content, n, bytes)]: every size from 1 to 330 for one repeated byte, a period of two and random bytes over four
    letters; 65216 to 65280 for the first two (their streams are a few hundred tokens)."""
    rng = np.random.default_rng(77)
    letters = bytes(rng.integers(0, 4, MEMBER_INPUT, dtype=np.uint8) + 65)
    whole = {"byte": b"a" * MEMBER_INPUT, "period2": b"ab" * (MEMBER_INPUT // 2), "letters": letters}
    out = []
    for content in SWEEP_CONTENTS:
        sizes = list(range(1, 331)) + (list(range(65216, 65281)) if content != "letters" else [])
        out += [(content, n, whole[content][:n]) for n in sizes if n not in SWEEP_HELD_ELSEWHERE]
    return out


def full_alphabets():
    """One member that uses all 256 literals, every length code up to 258 and every distance code up to 24577..32768.
    After the 256 byte values come 16 periodic pieces (period p, then a copy at distance p: the distance codes up to 193..256),
    then random anchors among zeros: one anchor copied down a chain, each copy shorter than the last and a chosen distance
    after it, and four anchors of their own for the distances over 8192.  The zeros between them repeat one 3-byte sequence
    only and cost next to nothing."""
    rng = np.random.default_rng(286)

    def fresh(n):
        return bytes(rng.integers(1, 256, n, dtype=np.uint8))

    lengths = list(LEN_BASE)
    out = bytearray(range(256))
    for p, ln in zip(DIST_BASE[:16], lengths[:15] + [258]):  # lengths 3..27, and one more of 258
        piece = fresh(p)
        out += (piece * (ln // p + 2))[:p + ln] + b"\0"
    far = ((24577 + 40, 258), (16385 + 40, 43), (12289 + 40, 35), (8193 + 40, 31))
    pieces, at = [], len(out)  # (offset, bytes) among the zeros
    for d, ln in far:
        a = fresh(260)
        pieces += [(at, a), (at + d, a[:ln])]
        at += 261
    anchor, at = fresh(260), at + 8
    pieces.append((at, anchor))
    for d, ln in zip(DIST_BASE[16:26], (227, 195, 163, 131, 115, 99, 83, 67, 59, 51)):
        at += d + 40
        pieces.append((at, anchor[:ln]))
    pieces.sort()
    buf = bytearray(pieces[-1][0] + 300)
    buf[:len(out)] = out
    end = len(out) - 1
    for o, piece in pieces:
        assert o > end, "two pieces overlap or touch"
        buf[o:o + len(piece)] = piece
        end = o + len(piece)
    assert len(buf) <= MEMBER_INPUT
    return bytes(buf)


def padded(data, seed):
    """data filled up to one member's input with random bytes over four letters drawn from this seed."""
    rng = np.random.default_rng(seed)
    return data + bytes(rng.integers(0, 4, MEMBER_INPUT - len(data), dtype=np.uint8) + 65)
