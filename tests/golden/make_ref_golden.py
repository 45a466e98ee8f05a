#!/usr/bin/env python3
"""Regenerates tests/golden/ref_*.npz: what THE REFERENCE ITSELF (haowenz/FEM v0.2) computes, recorded from a build of its
own sources (oracle/_ref/FEM_ref, its command line, and oracle/_ref/libfemref_fn.so, its functions one read at a time;
`make -C oracle ref`, which needs the reference's sources).  Nothing here is made by the oracle: the tests hold the oracle,
libfemhost and the kernels against these files where oracle/_ref is not built (tests/test_ref_parity.py,
tests/test_golden.py, tests/test_gpu_ref_parity.py), and against the live build where it is.

  ref_<case>.npz      CASES: small stored inputs (sequences, reads) and everything the reference gave for them — the five
                      counters, candidates per strand with the count before the additional q-gram filter, (ed, end) per
                      candidate, the records' fields, SHA-256 of the SAM file and of the index file
  ref_recorded.npz    SWEEP (inputs from libfemhost's seeded generator, not stored): counters and SHA-256 digests of the
                      same outcomes; INDEX_SHAPES: SHA-256 of `FEM_ref index` files; the lower-case reads: inputs and
                      which reads make the reference abort

Every comparison case stays inside the region where the reference's answer is defined (see defined_region below).

    python tests/golden/make_ref_golden.py
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fem_amd import host  # noqa: E402
from oracle import fem_oracle as fo  # noqa: E402
from oracle import ref_fem  # noqa: E402
from tests import util  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = os.path.join(HERE, "ref_recorded.npz")
K, STEP = 12, 3  # `FEM map` runs these whatever the index file says (src/FEM_map.c:67-68)

# Stored-input cases: at most 500 reads, at most 250 kbp of reference, each file below the largest older fixture.
CASES = {
    "ref_rand100_e3": dict(kind="rand", seed=101, seq_lens=[110_000], n_reads=400, L=100, e=3, a=1),
    # repeat-rich, three sequences with N runs, N's in the reads: strands with full groups of 8 candidates and remainders
    # of 1..7 (both Myers widths), reads with more than 64 records (klib's radix sort instead of its insertion sort)
    "ref_repeat150_e7": dict(kind="repeat", seed=102, n_reads=220, L=150, e=7, a=1, n_rate=0.003),
    "ref_short64_e2": dict(kind="rand", seed=103, seq_lens=[50_000, 30_000], n_reads=400, L=64, e=2, a=1),
    "ref_long300_e3": dict(kind="rand", seed=104, seq_lens=[90_000], n_reads=160, L=300, e=3, a=2),
    # several sequences (one shorter than a read, one shorter than k), reads from the first and last bases of each:
    # candidates dropped or kept at the borders by remove_out_ranged_candidates (src/filter.c:133-144)
    "ref_multi_ends": dict(kind="ends", seed=105, n_reads=300, L=100, e=3, a=0),
}

# Digest-only cases, inputs from libfemhost's generator (a pure function of the seed and the sizes).


def min_defined_length(e, a, k=K, step=STEP):
    """The smallest read length at which every phase group of the reference's seed selection has at least R * lg seeds,
    R = e + 1 + a, lg = ceil(k / step): g_min = (L - k + 1 - (step - 1)) // step >= R * lg.  With one seed fewer
    generate_optimal_prefix_qgram_for_group_seeding has a single column, picks nothing and its caller reads R
    uninitialised Seeds (src/filter.c:5-7, 30-41); with fewer still the column count wraps around."""
    lg = (k + step - 1) // step
    return step * (e + 1 + a) * lg + k + step - 2


def _sweep():
    out = {}
    for e in range(8):  # every e at its smallest defined length and one above
        for L in (min_defined_length(e, 1), min_defined_length(e, 1) + 1):
            out["e%d_a1_L%d" % (e, L)] = dict(seed=200 + 10 * e + (L & 1), seq_lens=[40_000, 9_000], n_reads=150, L=L, e=e, a=1)
    for a, e in ((0, 0), (0, 3), (2, 3), (2, 7), (0, 7)):
        for L in sorted({min_defined_length(e, a), 100 if e == 3 else min_defined_length(e, a) + 2}):
            out["e%d_a%d_L%d" % (e, a, L)] = dict(seed=300 + 10 * e + a, seq_lens=[40_000, 9_000], n_reads=150, L=L, e=e, a=a)
    for L, e in ((100, 3), (150, 5), (300, 3), (1000, 7)):
        out["long_e%d_L%d" % (e, L)] = dict(seed=400 + e + L, seq_lens=[70_000], n_reads=100, L=L, e=e, a=1)
    # more than one of the reference's input batches of 10 000 reads (src/FEM_map.c:151)
    out["batches_e2_L64"] = dict(seed=500, seq_lens=[80_000], n_reads=10_500, L=64, e=2, a=1, stages=False)
    return out


SWEEP = _sweep()

INDEX_SHAPES = [(12, 3), (12, 1), (10, 2), (13, 5), (7, 16), (5, 7), (2, 1)]


class Inputs:
    """Reference sequences and reads of one case, with the names and qualities the files carry."""

    def __init__(self, seqs, reads, names=None):
        self.seqs = [bytes(s) for s in seqs]
        self.reads = [bytes(r) for r in reads]
        self.names = names or ["chr%d" % (i + 1) for i in range(len(self.seqs))]
        self.rnames = ["r%d" % i for i in range(len(self.reads))]
        self.quals = ["".join(chr(33 + (7 * i + j) % 41) for j in range(len(r))) for i, r in enumerate(self.reads)]

    def arrays(self):
        lens = np.array([len(s) for s in self.seqs], np.uint32)
        rlen = np.array([len(r) for r in self.reads], np.uint64)
        return dict(in_text=np.frombuffer(b"".join(self.seqs), np.uint8), in_lens=lens,
                    in_bases=np.frombuffer(b"".join(self.reads), np.uint8),
                    in_offs=np.concatenate([[0], np.cumsum(rlen)]).astype(np.uint64))

    @classmethod
    def from_arrays(cls, z, prefix="in_"):  # (ref_recorded.npz: prefix "lower_")
        text, lens = z[prefix + "text"].tobytes(), z[prefix + "lens"]
        so = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
        bases, offs = z[prefix + "bases"].tobytes(), z[prefix + "offs"].astype(np.int64)
        return cls([text[so[i]:so[i + 1]] for i in range(len(lens))], [bases[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)])

    def write(self, directory):
        """(FASTA path, FASTQ path): the reference wrapped at 70 columns with a description after each name."""
        fa, fq = os.path.join(directory, "ref.fa"), os.path.join(directory, "reads.fq")
        with open(fa, "wb") as f:
            for n, s in zip(self.names, self.seqs):
                f.write(b">" + n.encode() + b" some description\n")
                for i in range(0, len(s), 70):
                    f.write(s[i:i + 70] + b"\n")
        with open(fq, "wb") as f:
            for n, r, q in zip(self.rnames, self.reads, self.quals):
                f.write(b"@" + n.encode() + b" 1:N:0\n" + r + b"\n+\n" + q.encode() + b"\n")
        return fa, fq


def make_inputs(case):
    """A stored-input case's inputs from scratch (what the committed fixture stores)."""
    rng = np.random.default_rng(case["seed"])
    L, e = case["L"], case["e"]
    if case["kind"] == "rand":
        seqs = [util.rand_seq(rng, n) for n in case["seq_lens"]]
        reads = util.make_reads(rng, seqs, case["n_reads"], L, e)
    elif case["kind"] == "repeat":
        seqs = util.repeat_rich_reference(rng, n_seq=3, unit_len=300, n_units=3, copies=60, spacer=200)
        reads = util.make_reads(rng, seqs, case["n_reads"], L, e, n_rate=case["n_rate"])
    else:  # "ends"
        seqs = [util.rand_seq(rng, 30_000), util.rand_seq(rng, 60), util.rand_seq(rng, 7), util.rand_seq(rng, 20_011),
                bytes(util.rand_seq(rng, 400)) + b"N" * 40 + util.rand_seq(rng, 5_000)]
        long_ones = [s for s in seqs if len(s) > L + 4 * e + 8]
        reads = []
        for i in range(case["n_reads"]):
            s = long_ones[i % len(long_ones)]
            d = int(rng.integers(0, 2 * e + 3))  # distance of the read's window from the sequence's border
            start = d if (i // len(long_ones)) % 2 == 0 else len(s) - (L + e) - d
            r = util.mutate(rng, s[start:start + L + e], int(rng.integers(0, e + 1)))[:L]
            r = r + util.rand_seq(rng, L - len(r))
            reads.append(util.revcomp(r) if rng.random() < 0.5 else r)
    return Inputs(seqs, reads)


def stored_inputs(name):
    return Inputs.from_arrays(np.load(os.path.join(HERE, name + ".npz")))


def sweep_inputs(case):
    text, off, lens = host.synth_reference(case["seed"], case["seq_lens"], threads=4)
    bases, offs = host.synth_reads(case["seed"], text, off, lens, case["n_reads"], case["L"], case["e"], threads=4)
    L = case["L"]
    raw = bases.tobytes()
    return Inputs([text[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, lens)],
                  [raw[i * L:(i + 1) * L] for i in range(case["n_reads"])])


def lowercase_inputs():
    """About 40 reads on a reference with a soft-masked (lower-case) stretch: some inside it, some across its borders,
    some outside; a few lower-case reads on upper-case reference."""
    rng = np.random.default_rng(77)
    s = bytearray(util.rand_seq(rng, 6_000))
    s[2_000:2_600] = bytes(s[2_000:2_600]).lower()
    reads = []
    for i in range(40):
        start = [1_900, 1_950, 2_100, 2_300, 2_550, 2_580, 400, 4_000][i % 8] + int(rng.integers(0, 40))
        r = util.mutate(rng, bytes(s[start:start + 103]).upper(), i % 4)[:100]
        r = r + util.rand_seq(rng, 100 - len(r))
        if i % 8 >= 6 and i % 3 == 0:
            r = r.lower()
        reads.append(util.revcomp(r.upper()) if i % 5 == 0 else r)
    return Inputs([bytes(s)], reads)


# ---------------------------------------------------------------------------------------------- outcomes
def sha(data):
    return np.frombuffer(hashlib.sha256(data).digest(), np.uint8)


def defined_region(inp, e, a):
    """True where every read of the case is upper-case ACGTN and at or above min_defined_length: the region in which the
    reference's answer is defined.  Every comparison case asserts this (and no 0x8000 flag from the oracle)."""
    ok_chars = set(b"ACGTN")
    return all(len(r) >= min_defined_length(e, a) and set(r) <= ok_chars for r in inp.reads) and \
        all(set(s) <= ok_chars for s in inp.seqs)


def parse_sam(text, inp):
    """The record fields of a SAM text of this case's reads: arrays named as oracle.fem_oracle.MapResult names them, plus
    r_mapq.  QNAME, RNEXT, PNEXT, TLEN, SEQ and QUAL are checked against the inputs here."""
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(inp.names, inp.seqs))
    assert text.startswith(header), "@SQ lines"
    tid_of = {n: i for i, n in enumerate(inp.names)}
    n = len(inp.reads)
    per_read = np.zeros(n, np.int64)
    flag, tid, pos, nm, mapq, cig, cig_off, md, md_off = [], [], [], [], [], [], [0], [], [0]
    last = -1
    for line in text[len(header):].splitlines():
        f = line.split("\t")
        assert len(f) == 13 and f[0][0] == "r", line
        r = int(f[0][1:])
        assert r >= last, "records follow the order of the reads"
        primary = r != last
        last = r
        assert f[6:9] == ["*", "0", "0"]
        assert (f[9], f[10]) == ((inp.reads[r].decode().upper(), inp.quals[r]) if primary else ("*", "*")), line
        per_read[r] += 1
        flag.append(int(f[1])), tid.append(tid_of[f[2]]), pos.append(int(f[3]) - 1), mapq.append(int(f[4]))
        num = ""
        for ch in f[5]:
            if ch.isdigit():
                num += ch
            else:
                cig.append(int(num) << 4 | "MIDNSHP=X".index(ch))
                num = ""
        cig_off.append(len(cig))
        assert f[11].startswith("NM:i:") and f[12].startswith("MD:Z:")
        nm.append(int(f[11][5:]))
        md.append(f[12][5:].encode())
        md_off.append(md_off[-1] + len(md[-1]))
    return dict(rec_off=np.concatenate([[0], np.cumsum(per_read)]).astype(np.uint64), r_flag=np.array(flag, np.uint16),
                r_tid=np.array(tid, np.uint32), r_pos=np.array(pos, np.uint32), r_nm=np.array(nm, np.uint8),
                r_mapq=np.array(mapq, np.uint8), cig_off=np.array(cig_off, np.uint64), cig=np.array(cig, np.uint32),
                md_off=np.array(md_off, np.uint64), md=np.frombuffer(b"".join(md), np.uint8))


def reference_outcome(inp, e, a, stages=True):
    """What the reference's build gives for these inputs: FEM_ref index + map -t 1 (index file, SAM file, counters) and,
    through libfemref_fn.so, the candidates and (ed, end) per strand.  Needs oracle/_ref."""
    with tempfile.TemporaryDirectory() as d:
        fa, fq = inp.write(d)
        ix, sam = os.path.join(d, "ref.idx"), os.path.join(d, "out.sam")
        ref_fem.cli_index(K, STEP, fa, ix)
        r, counters = ref_fem.cli_map(e, a, fa, ix, fq, sam)
        assert r.returncode == 0 and counters is not None, r.stderr.decode(errors="replace")[-2000:]
        text = open(sam).read()
        out = dict(stats=counters, index_sha256=sha(open(ix, "rb").read()), sam_sha256=sha(text.encode()), sam_text=text)
        out.update(parse_sam(text, inp))
        if stages:
            with ref_fem.RefFem(fa) as rf:
                rf.load_index(ix)
                assert rf.load_reads(fq, len(inp.reads)) == len(inp.reads)
                cand_off, cands, pre, v_ed, v_end = [0], [], [], [], []
                for i in range(len(inp.reads)):
                    for direction in (0, 1):
                        c, p = rf.candidates(e, a, i, direction)
                        ed, end, dr, mc = rf.verify(e, a, i, direction, c)
                        assert np.all(dr == direction) and np.all(np.diff(np.searchsorted(c, mc)) > 0)  # candidate order
                        sed, send = np.full(len(c), 0xFF, np.uint8), np.zeros(len(c), np.int16)
                        at = np.searchsorted(c, mc)
                        assert np.array_equal(c[at], mc)
                        sed[at], send[at] = ed, end
                        cands.append(c), pre.append(p), v_ed.append(sed), v_end.append(send)
                        cand_off.append(cand_off[-1] + len(c))
                out.update(cand_off=np.array(cand_off, np.uint64), cands=np.concatenate(cands).astype(np.uint64),
                           pre=np.array(pre, np.uint32), v_ed=np.concatenate(v_ed).astype(np.uint8),
                           v_end=np.concatenate(v_end).astype(np.int16))
        return out


def oracle_outcome(inp, e, a, with_result=False):
    """The same outcome from the oracle (oracle/fem_oracle.c), under the same names."""
    from tests.cases import expected_sam
    ref = fo.Reference(inp.seqs)
    idx = fo.OracleIndex(ref, K, STEP)
    res = fo.map_reads(ref, idx, fo.ReadBatch(inp.reads), e=e, a=a, k=K, step=STEP)
    with tempfile.TemporaryDirectory() as d:
        idx.save(os.path.join(d, "o.idx"))
        index_bytes = open(os.path.join(d, "o.idx"), "rb").read()
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(inp.names, inp.seqs))
    text = header + expected_sam(inp.names, inp.reads, inp.rnames, inp.quals, res)
    v_end = res.v_end.copy()
    v_end[res.v_ed == 0xFF] = 0
    out = dict(stats=res.stats, index_sha256=sha(index_bytes), sam_sha256=sha(text.encode()), sam_text=text,
               rec_off=res.rec_off, r_flag=res.r_flag, r_tid=res.r_tid, r_pos=res.r_pos, r_nm=res.r_nm,
               r_mapq=np.full(len(res.r_flag), 255, np.uint8), cig_off=res.cig_off, cig=res.cig, md_off=res.md_off,
               md=res.md, cand_off=res.cand_off, cands=res.cands, pre=res.pre, v_ed=res.v_ed, v_end=v_end)
    return (out, res, ref, idx) if with_result else out


STAGE_KEYS = ["cand_off", "cands", "pre", "v_ed", "v_end"]
RECORD_KEYS = ["rec_off", "r_flag", "r_tid", "r_pos", "r_nm", "r_mapq", "cig_off", "cig", "md_off", "md"]
STORED_KEYS = ["stats", "index_sha256", "sam_sha256"] + STAGE_KEYS + RECORD_KEYS


def blob_sha(out, keys):
    """SHA-256 of an outcome's arrays under these names (each name, then the array's bytes)."""
    return sha(b"".join(k.encode() + np.ascontiguousarray(out[k]).tobytes() for k in keys))


def digests(out, stages=True):
    """uint8[3 or 4, 32]: SHA-256 of the index file, of the SAM file, of the records' arrays and (stages) of the
    per-strand arrays of an outcome."""
    rows = [out["index_sha256"], out["sam_sha256"], blob_sha(out, RECORD_KEYS)]
    if stages:
        rows.append(blob_sha(out, STAGE_KEYS))
    return np.stack(rows)


def lowercase_aborts(inp, e=3, a=1):
    """uint8[n_reads]: 1 where FEM_ref, given that read alone, dies by SIGABRT (an assert of the reference)."""
    out = np.zeros(len(inp.reads), np.uint8)
    with tempfile.TemporaryDirectory() as d:
        fa, _ = inp.write(d)
        ix = os.path.join(d, "ref.idx")
        ref_fem.cli_index(K, STEP, fa, ix)
        for i, r in enumerate(inp.reads):
            fq = os.path.join(d, "one.fq")
            with open(fq, "wb") as f:
                f.write(b"@" + inp.rnames[i].encode() + b"\n" + r + b"\n+\n" + inp.quals[i].encode() + b"\n")
            p, counters = ref_fem.cli_map(e, a, fa, ix, fq, os.path.join(d, "one.sam"))
            assert p.returncode in (0, -6), (i, p.returncode, p.stderr.decode(errors="replace")[-500:])
            assert (p.returncode == 0) == (counters is not None)
            out[i] = p.returncode == -6
    return out


def index_buffer_in_bounds(seq_lens, k, step):
    """construct_index collects its seeds in a buffer of num_bases / step + 1 entries (src/index.c:59): enough for one
    sequence, but with several sequences and step > k their rounded-up counts can add up to more, and the reference writes
    past the buffer.  True where it does not: the index tests keep to such references."""
    return sum((n - k) // step + 1 for n in seq_lens if n >= k) <= sum(seq_lens) // step + 1


def index_inputs():
    """The reference of the index tests: several sequences, one shorter than every k (1 base), one shorter than most
    (7 bases), N runs, a soft-masked stretch; lengths at which index_buffer_in_bounds holds for every shape."""
    rng = np.random.default_rng(88)
    a = bytearray(util.rand_seq(rng, 9_000))
    a[3_000:3_400] = bytes(a[3_000:3_400]).lower()
    b = util.rand_seq(rng, 700) + b"N" * 33 + util.rand_seq(rng, 1_500) + b"N" + util.rand_seq(rng, 19)
    inp = Inputs([bytes(a), util.rand_seq(rng, 7), util.rand_seq(rng, 1), b, util.rand_seq(rng, 4_003)], [])
    assert all(index_buffer_in_bounds([len(s) for s in inp.seqs], k, step) for k, step in INDEX_SHAPES)
    return inp


def index_file_sha(inp, k, step):
    with tempfile.TemporaryDirectory() as d:
        fa, _ = inp.write(d)
        ix = os.path.join(d, "r.idx")
        ref_fem.cli_index(k, step, fa, ix)
        return sha(open(ix, "rb").read())


if __name__ == "__main__":
    assert ref_fem.available(), "needs oracle/_ref (make -C oracle ref, with the reference's sources present)"
    for name, case in CASES.items():
        inp = make_inputs(case)
        assert defined_region(inp, case["e"], case["a"]), name
        got = reference_outcome(inp, case["e"], case["a"])
        per_strand, per_read = np.diff(got["cand_off"].astype(np.int64)), np.diff(got["rec_off"].astype(np.int64))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **inp.arrays(), **{k: got[k] for k in STORED_KEYS})
        print(name, "stats", got["stats"].tolist(), "records", len(got["r_flag"]), "max records per read", int(per_read.max()),
              "strands with >= 8 candidates", int((per_strand >= 8).sum()), "remainders", sorted(set((per_strand[per_strand >= 8] % 8).tolist())),
              "bytes", os.path.getsize(os.path.join(HERE, name + ".npz")))
    rec = {}
    for key, case in SWEEP.items():
        inp = sweep_inputs(case)
        assert defined_region(inp, case["e"], case["a"]), key
        got = reference_outcome(inp, case["e"], case["a"], stages=case.get("stages", True))
        rec["sweep/%s/stats" % key] = got["stats"]
        rec["sweep/%s/digests" % key] = digests(got, stages=case.get("stages", True))
        print(key, got["stats"].tolist())
    ii = index_inputs()
    for k, step in INDEX_SHAPES:
        rec["index/%d_%d" % (k, step)] = index_file_sha(ii, k, step)
    low = lowercase_inputs()
    rec.update({"lower_" + k[3:]: v for k, v in low.arrays().items()})
    rec["lower_aborts"] = lowercase_aborts(low)
    print("lower-case reads that abort:", rec["lower_aborts"].tolist())
    np.savez_compressed(RECORDED, **rec)
    print("ref_recorded.npz", os.path.getsize(RECORDED), "bytes")
