"""BAM output without a GPU: the model of tests/bam_model.py against the specification, fem_bam_header against the model,
and FEM map's --bam refusals."""
import gzip
import struct
import zlib

import numpy as np
import pytest

from fem_amd import host
from tests import bam_model as bm
from tests.harness import run_fem

REFS = [b"chr1", b"chrX_long_name"]


@pytest.mark.parametrize("line", [
    b"r1\t0\tchr1\t100\t255\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\tMD:Z:10",
    b"r2/1\t16\tchr1\t1\t255\t3M1I4M2D2M\t*\t0\t0\tACGTACGTAC\t#$%&'()*+,\tNM:i:3\tMD:Z:7^AC2",
    b"r3\t256\tchrX_long_name\t5000\t255\t50M\t*\t0\t0\t*\t*\tNM:i:1\tMD:Z:20G29",
    b"p1\t99\tchr1\t200\t255\t5M\t=\t400\t205\tAAAAA\tIIIII\tNM:i:0\tMD:Z:5",
    b"p1\t147\tchr1\t400\t255\t5M\t=\t200\t-205\tCCCCC\tIIIII\tNM:i:0\tMD:Z:5",
    b"p2\t65\tchr1\t300\t255\t4M\tchrX_long_name\t77\t0\tGGGG\t!!!!\tNM:i:0\tMD:Z:4",
    b"r4\t0\tchr1\t7\t255\t6M\t*\t0\t0\tACGTNN\t*\tNM:i:2\tMD:Z:4A0C0",
    b"r5\t0\tchr1\t7\t255\t*\t*\t0\t0\t*\t*\tNM:i:0\tMD:Z:",
    b"r6\t0\tchr1\t9\t255\t9M\t*\t0\t0\tRYKM=SWBN\tIIIIIIIII\tNM:i:9\tMD:Z:0A0A0A0A0A0A0A0A0A0",
])
def test_encode_decode_round_trip(line):
    rec = bm.encode(line, REFS)
    back, size = bm.decode(rec, REFS)
    assert size == len(rec) and back == line
    (bs,) = struct.unpack_from("<i", rec)
    assert bs == len(rec) - 4


def test_lower_case_and_unknown_letters_take_the_round_trip_letters():
    line = b"r\t0\tchr1\t1\t255\t8M\t*\t0\t0\tacgtnrx.\tIIIIIIII\tNM:i:0\tMD:Z:8"
    back, _ = bm.decode(bm.encode(line, REFS), REFS)
    assert back.split(b"\t")[9] == b"ACGTNRNN"


def test_record_fields_by_hand():
    line = b"abc\t16\tchrX_long_name\t17000\t255\t2M1D3M\t*\t0\t0\tACGTA\t!!!!!\tNM:i:1\tMD:Z:2^A3"
    rec = bm.encode(line, REFS)
    tid, pos0, l_name, mapq, bin_, n_ops, flag, l_seq, ntid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    assert (tid, pos0, l_name, mapq, n_ops, flag, l_seq, ntid, npos, tlen) == (1, 16999, 4, 255, 3, 16, 5, -1, -1, 0)
    assert bin_ == bm.reg2bin(16999, 16999 + 6) == 4682  # 16999 >> 14 = 1
    assert rec[36:40] == b"abc\0"  # (after block_size and the 32 bytes of fixed fields)
    assert struct.unpack_from("<3I", rec, 40) == (2 << 4 | 0, 1 << 4 | 2, 3 << 4 | 0)
    assert rec[52:55] == bytes([0x12, 0x48, 0x10])  # A C G T A: 1 2 4 8 1, padded with 0
    assert rec[55:60] == b"\0" * 5 and rec[60:] == b"NMC\x01MDZ2^A3\0"


def test_reg2bin_against_the_specification():
    assert bm.reg2bin(-1, 0) == 4680  # unplaced: (2^15 - 1) / 7 + (-1 >> 14) in the specification's arithmetic
    assert bm.reg2bin(0, 1) == 4681
    for shift in (14, 17, 20, 23, 26):
        b = 1 << shift
        assert bm.reg2bin(b - 1, b) == 4681 + ((b - 1) >> 14)  # one base: always the finest level
        assert bm.reg2bin(b, b + 1) == 4681 + (b >> 14)
        assert bm.reg2bin(0, b + 1) == {14: 585, 17: 73, 20: 9, 23: 1, 26: 0}[shift]  # one base past: the next level up
    assert bm.reg2bin((1 << 14) - 1, (1 << 14) + 1) == 585       # across a 2^14 boundary: the 2^17 level
    assert bm.reg2bin((1 << 17) - 1, (1 << 17) + 1) == 73
    assert bm.reg2bin((1 << 20) - 1, (1 << 20) + 1) == 9
    assert bm.reg2bin((1 << 23) - 1, (1 << 23) + 1) == 1
    assert bm.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    assert bm.reg2bin(0, 1 << 29) == 0


def _ref(names, lens):
    text = np.zeros(max(1, min(sum(lens), 1 << 16)), np.uint8)
    off = np.zeros(len(lens), np.uint64)
    return host.TailReference(text, off, np.array(lens, np.uint64).astype(np.uint32), names=names)


@pytest.mark.parametrize("names,lens", [(["chr1"], [1000]), (["c%d_%s" % (i, "n" * (i * 37 % 300)) for i in range(500)],
                                                            [1 + 7919 * i for i in range(500)]),
                                        (["x" * 1000, "y"], [(1 << 31) - 1, 1])])
def test_bam_header_equals_the_model(names, lens):
    ref = _ref(names, lens)
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(names, lens)).encode()
    assert host.sam_header(ref).encode() == text
    assert host.bam_header(ref) == bm.header(text, [n.encode() for n in names], lens)


def test_bam_header_refuses_a_sequence_of_2_31_bases():
    with pytest.raises(ValueError):
        host.bam_header(_ref(["chr1", "big"], [10, 1 << 31]))


def test_bgzf_parser_on_zlib_members():
    """The parser itself, on members written with zlib (so that it is not only ever checked against the device)."""
    payload = bytes(range(256)) * 600
    members = b""
    for i in range(0, len(payload), bm.MEMBER_INPUT):
        chunk = payload[i:i + bm.MEMBER_INPUT]
        c = zlib_raw(chunk)
        members += (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(c) + 8 - 1) + c +
                    struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    parsed = bm.parse_bgzf(members + bm.BGZF_EOF)
    assert b"".join(p for p, _, _ in parsed) == payload and gzip.decompress(members + bm.BGZF_EOF) == payload
    with pytest.raises(AssertionError):
        bm.parse_bgzf(members)  # no EOF block


def zlib_raw(b):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return c.compress(b) + c.flush()


def test_cli_bam_usage_and_refusals():
    import __graft_entry__ as g
    g.build()
    r = run_fem("map", "-h")
    assert r.returncode == 0 and b"--bam" in r.stderr
    base = ("map", "--ref", "a", "--index", "b", "--read1", "c", "-o", "d")
    for bad in ("--bam=2", "--bam=x", "--bam=", "--bam=01"):
        r = run_fem(*(base + (bad,)))
        assert r.returncode == 1 and b"Wrong BAM compression level (0-1)." in r.stderr, bad
    for var in ("FEM_HOST_TAIL", "FEM_HOST_FORMAT", "FEM_HOST_QUALS"):
        r = run_fem(*(base + ("--bam",)), env={var: "1"})
        assert r.returncode == 1 and (b"--bam is not supported with %s=1" % var.encode()) in r.stderr, var
        assert b"Loaded index" not in r.stderr
