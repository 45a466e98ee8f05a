"""An independent model of BAM output, from the SAM/BAM specification (§4.1 BGZF, §4.2 BAM, §5.3 bins), on struct, zlib and
gzip only: SAM line <-> BAM record, reg2bin, the BAM header, a BGZF member parser, and payload generators."""
import re
import struct
import zlib

import numpy as np

SEQ_CODES = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=XB"
BGZF_EOF = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MEMBER_INPUT = 65280


def reg2bin(beg, end):
    """Spec §5.3: the bin of [beg, end), 0-based, end exclusive."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def _seq_code(ch):
    i = SEQ_CODES.find(bytes([ch]).upper())
    return 15 if i < 0 else i


def encode(line, ref_names):
    """One SAM line (bytes, no newline) -> one BAM record (block_size included).  ref_names: list of bytes."""
    ids = {n: i for i, n in enumerate(ref_names)}
    f = line.split(b"\t")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    tid = -1 if rname == b"*" else ids[rname]
    pos0 = int(pos) - 1
    ops = [] if cigar == b"*" else [(int(n), CIGAR_OPS.index(o)) for n, o in re.findall(rb"(\d+)([MIDNSHP=XB])", cigar)]
    span = sum(n for n, o in ops if o in (0, 2, 3, 7, 8))
    bin_ = reg2bin(pos0, pos0 + (span if span else 1)) if pos0 >= 0 else 4680
    ntid = -1 if rnext == b"*" else tid if rnext == b"=" else ids[rnext]
    l_seq = 0 if seq == b"*" else len(seq)
    codes = [_seq_code(c) for c in (b"" if seq == b"*" else seq)]
    if l_seq % 2:
        codes.append(0)
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    q = b"\xff" * l_seq if qual == b"*" else bytes(c - 33 for c in qual)
    aux = b""
    for t in f[11:]:
        tag, typ, val = t.split(b":", 2)
        if typ == b"i":
            v = int(val)
            aux += tag + (b"C" + struct.pack("<B", v) if 0 <= v <= 255 else b"i" + struct.pack("<i", v))
        elif typ == b"Z":
            aux += tag + b"Z" + val + b"\0"
        else:
            raise ValueError("tag type %r not modelled" % typ)
    body = struct.pack("<iiBBHHHiiii", tid, pos0, len(qname) + 1, int(mapq), bin_, len(ops), int(flag), l_seq, ntid,
                       int(pnext) - 1, int(tlen))
    body += qname + b"\0" + b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + packed + q + aux
    return struct.pack("<i", len(body)) + body


def decode(rec, ref_names):
    """One BAM record -> (SAM line bytes, record size)."""
    (bs,) = struct.unpack_from("<i", rec, 0)
    tid, pos0, l_name, mapq, bin_, n_ops, flag, l_seq, ntid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    p = 36
    qname = rec[p:p + l_name - 1]
    assert rec[p + l_name - 1] == 0
    p += l_name
    ops = struct.unpack_from("<%dI" % n_ops, rec, p)
    p += 4 * n_ops
    cigar = b"".join(b"%d%c" % (x >> 4, CIGAR_OPS[x & 15]) for x in ops) or b"*"
    sb = (l_seq + 1) // 2
    seq = bytes(SEQ_CODES[(rec[p + i // 2] >> (4 * (1 - i % 2))) & 15] for i in range(l_seq)) or b"*"
    p += sb
    qual = rec[p:p + l_seq]
    p += l_seq
    qual = b"*" if l_seq == 0 or qual[0] == 0xFF else bytes(c + 33 for c in qual)
    tags = []
    end = 4 + bs
    while p < end:
        tag, typ = rec[p:p + 2], rec[p + 2:p + 3]
        p += 3
        if typ in b"cCsSiI":
            fmt = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}[typ]
            (v,) = struct.unpack_from(fmt, rec, p)
            p += struct.calcsize(fmt)
            tags.append(tag + b":i:%d" % v)
        elif typ == b"Z":
            z = rec.index(b"\0", p)
            tags.append(tag + b":Z:" + rec[p:z])
            p = z + 1
        else:
            raise ValueError("tag type %r not modelled" % typ)
    assert p == end
    rname = b"*" if tid < 0 else ref_names[tid]
    rnext = b"*" if ntid < 0 else b"=" if ntid == tid else ref_names[ntid]
    fields = [qname, b"%d" % flag, rname, b"%d" % (pos0 + 1), b"%d" % mapq, cigar, rnext, b"%d" % (npos + 1), b"%d" % tlen, seq,
              qual] + tags
    return b"\t".join(fields), end


def header(text, names, lens):
    """The uncompressed BAM header: magic, l_text, text, n_ref, (l_name, name NUL, l_ref) per sequence."""
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(names))
    for n, ln in zip(names, lens):
        out += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", ln)
    return out


def records(payload):
    """Split a run of BAM records into the records."""
    out, p = [], 0
    while p < len(payload):
        (bs,) = struct.unpack_from("<i", payload, p)
        out.append(payload[p:p + 4 + bs])
        p += 4 + bs
    assert p == len(payload)
    return out


def sam_to_bam_payload(sam_text, ref_names):
    return b"".join(encode(l, ref_names) for l in sam_text.split(b"\n") if l)


def bam_payload_to_sam(payload, ref_names):
    return b"".join(decode(r, ref_names)[0] + b"\n" for r in records(payload))


def parse_bgzf(data, eof=True):
    """Check every member (magic, FEXTRA with one BC field, BSIZE, size <= 65536, raw deflate that ends the member, CRC-32,
    ISIZE) and, with eof, the 28-byte EOF block at the end.  Returns [(payload, member size, BTYPE of its first block)]."""
    out, i = [], 0
    while i < len(data):
        assert data[i:i + 4] == b"\x1f\x8b\x08\x04", "gzip magic / FEXTRA at %d" % i
        (xlen,) = struct.unpack_from("<H", data, i + 10)
        assert xlen == 6 and data[i + 12:i + 14] == b"BC" and struct.unpack_from("<H", data, i + 14)[0] == 2
        size = struct.unpack_from("<H", data, i + 16)[0] + 1
        assert size <= 65536 and i + size <= len(data)
        m = data[i:i + size]
        d = zlib.decompressobj(-15)
        raw = d.decompress(m[18:-8])
        assert d.eof and not d.unused_data, "deflate data does not end the member"
        crc, isize = struct.unpack("<II", m[-8:])
        assert zlib.crc32(raw) == crc and len(raw) == isize
        out.append((raw, size, (m[18] >> 1) & 3))
        i += size
    if eof:
        assert data.endswith(BGZF_EOF), "no BGZF EOF block"
        assert out and out[-1][0] == b"" and out[-1][1] == 28
        out = out[:-1]
    return out


# ---- payload generators ----
def illumina_quals(rng, L):
    """Illumina-like 4-bin qualities."""
    return bytes(33 + rng.choice([2, 12, 23, 37], size=L, p=[0.03, 0.07, 0.15, 0.75]).astype(np.uint8))


def random_walk_quals(rng, L):
    """Unbinned qualities: a random walk over 2..41."""
    q = np.empty(L, np.int64)
    v = int(rng.integers(30, 42))
    for i in range(L):
        v = min(41, max(2, v + int(rng.integers(-3, 4))))
        if rng.random() < 0.01:
            v = 2
        q[i] = v
    return bytes((q + 33).astype(np.uint8))


def synthetic_sam(rng, n, L, profile, ref_names=(b"chr1", b"chr2")):
    """n SAM lines of L-base reads that look like FEM map's, with qualities of the given profile ("illumina" / "walk")."""
    gen = illumina_quals if profile == "illumina" else random_walk_quals
    lines = []
    pos = 1000
    for i in range(n):
        pos += int(rng.integers(0, 400))
        seq = bytes(rng.choice(list(b"ACGT"), size=L).astype(np.uint8))
        nm = int(rng.integers(0, 4))
        md = b"%d" % L if nm == 0 else b"%dA%d" % (L // 2, L - L // 2 - 1)
        lines.append(b"\t".join([b"SRR0000001.%d" % (i + 1), b"%d" % (16 * int(rng.integers(0, 2))), ref_names[0],
                                 b"%d" % pos, b"255", b"%dM" % L, b"*", b"0", b"0", seq, gen(rng, L), b"NM:i:%d" % nm,
                                 b"MD:Z:" + md]))
    return b"\n".join(lines) + b"\n"
