"""What the tests do with a device or with the FEM binary, once: the path of the binary and its runner, the parser of its
counters, a handle with reference, names and index uploaded, "stage reads and text, map, fetch the SAM text", and the
comparisons of the device's arrays, texts and BAM with what tests/cases.py and the models expect.  Functions take explicit
arguments; a test module that keeps its case in a dict wraps them in a line of its own.  No test module imports another: what
two of them share lives here or in tests/cases.py."""
import contextlib
import gzip
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

from oracle import fem_oracle as fo
from tests import bam_model as bm
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEM = os.path.join(ROOT, "fem_amd", "csrc", "FEM")


# ---- the command line ----

def run_fem(*args, env=None, timeout=900, text=False):
    """FEM with these arguments, `env` on top of the environment -> the completed process (stdout and stderr as bytes, as
    str with text)."""
    full = dict(os.environ, **env) if env else None
    return subprocess.run([FEM] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=full,
                          text=text)


def build_index(fa, idx_path, k=12, step=3):
    """FEM index, which must succeed."""
    r = run_fem("index", k, step, fa, idx_path)
    assert r.returncode == 0, r.stderr.decode()


def counters(stderr):
    """The "The number of ..." lines of FEM map's stderr (str or bytes)."""
    if isinstance(stderr, bytes):
        stderr = stderr.decode()
    return [l for l in stderr.splitlines() if l.startswith("The number of")]


def counter(stderr, what):
    """The values of the counter lines "The number of <what>: n"."""
    return [int(l.rsplit(": ", 1)[1]) for l in counters(stderr) if l.startswith("The number of " + what + ":")]


# ---- a handle and a batch through it ----

def device_with_env(**env):
    """A handle opened with these environment switches set; the environment is restored afterwards."""
    from fem_amd import Device
    was = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Device(0)
    finally:
        for k, v in was.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def library_stderr():
    """What the library writes to stderr inside the block (C stdio on file descriptor 2: the FEM_TIMELINE lines) -> a list
    that holds the text once the block has ended."""
    out = []
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            yield out
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            out.append(f.read().decode())


def open_device(seqs, names, idx=None, k=12, step=3):
    """A handle on GPU 0 with the reference, its names (None: none) and the oracle's index uploaded -> dev, ref, idx."""
    from fem_amd import Device
    ref = fo.Reference(seqs)
    if idx is None:
        idx = fo.OracleIndex(ref, k, step)
    dev = Device(0)
    dev.upload_reference(seqs)
    if names is not None:
        dev.upload_reference_names(names)
    dev.upload_index(k, step, idx.lookup, idx.occ[:idx.n_occ])
    return dev, ref, idx


def open_reference(seed, repeats, second=60_000, name_pad=None):
    """cases.reference from a generator of this seed, on a handle -> rng, dev, ref, idx, seqs, names."""
    rng = np.random.default_rng(seed)
    seqs, names = cases.reference(rng, repeats, second, name_pad)
    dev, ref, idx = open_device(seqs, names)
    return rng, dev, ref, idx, seqs, names


def open_sam_case(seed, e, L, n_reads, repeats, odd):
    """cases.sam_case on a handle -> dev, ref, idx, seqs, names, reads, rnames, quals."""
    ref, idx, seqs, names, reads, rnames, quals = cases.sam_case(seed, e, L, n_reads, repeats, odd)
    return open_device(seqs, names, idx)[0], ref, idx, seqs, names, reads, rnames, quals


def stage_and_map(dev, reads, rnames, quals, e, slot=0, quals_on_host=False, packed=False):
    """Reads, names and qualities into the slot's staging and the mapping started -> what fetch_sam needs to fill the
    qualities in where they stay on the host: (quals, offsets), else (None, None)."""
    from fem_amd import device
    batch = fo.ReadBatch(reads)
    q = np.frombuffer("".join(quals).encode("latin-1"), np.uint8)
    if packed:  # the 2-bit form through the staging (fem_dev_commit_stage_packed)
        n, L = len(reads), len(reads[0])
        hb, _ = dev.acquire_stage(n, n * L, slot=slot)
        n_exc = device.pack_reads(batch.bases, n, L, hb)
        dev.commit_stage_packed(n, L, n_exc, slot=slot)
    else:
        dev.stage_reads(batch.bases, batch.off, slot=slot)
    if packed:
        assert dev.stage_info(slot)[1]
    elif len(set(len(r) for r in reads)) > 1:
        assert not dev.stage_info(slot)[1]  # (mates of unequal lengths: as characters)
    dev.stage_text(q, rnames, slot=slot, quals_on_host=quals_on_host)
    dev.map_staged(e=e, slot=slot)
    return (q, batch.off) if quals_on_host else (None, None)


def fetch_sam(dev, reads, rnames, quals, e, slot=0, quals_on_host=False, packed=False):
    """stage_and_map and the slot's SAM text -> (text, n_records, n_asserted, stats), as Device.fetch_sam."""
    q, off = stage_and_map(dev, reads, rnames, quals, e, slot, quals_on_host, packed)
    return dev.fetch_sam(slot=slot, quals=q, offsets=off)


def run_packed(dev, reads, L, e, k, step):
    """A batch of equal-length reads staged in the 2-bit form, seeded and verified -> per-strand arrays and the statistics."""
    from fem_amd import device
    n = len(reads)
    bases = np.frombuffer(b"".join(reads), np.uint8)
    hb, _ = dev.acquire_stage(n, n * L)
    n_exc = device.pack_reads(bases, n, L, hb)
    assert n_exc == sum(sum(1 for c in r if c not in b"ACGT") for r in reads)
    dev.commit_stage_packed(n, L, n_exc)
    assert dev.stage_info()[1]
    dev.map_staged(e=e, k=k, step=step)
    got = dev.fetch()
    return got.per_strand() + (got.stats,)


# ---- comparisons ----

def first_difference(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
    return "line %d of %d / %d: got %r want %r" % (k, len(g) - 1, len(w) - 1, g[k:k + 1], w[k:k + 1])


def same_text(got, want):
    if got != want:  # (the first difference, not two texts of megabytes)
        raise AssertionError(first_difference(got, want))


def assert_same(want, got):
    off, cand, ed, end = got.per_strand()
    assert np.array_equal(off, want.cand_off), "candidate counts per (read, strand)"
    assert np.array_equal(cand, want.cands), "candidate locations"
    assert np.array_equal(ed, want.v_ed), "edit distances / accept set"
    assert np.array_equal(end[ed != 0xFF], want.v_end[want.v_ed != 0xFF]), "end offsets"
    assert np.array_equal(got.stats, want.stats), (got.stats, want.stats)


def assert_same_records(want, got):
    assert np.array_equal(got.rec_begin, want.rec_off), "records per read"
    assert np.array_equal(got.flag, want.r_flag), "FLAG"
    assert np.array_equal(got.tid, want.r_tid), "reference id"
    assert np.array_equal(got.pos0, want.r_pos), "POS"
    assert np.array_equal(got.nm, want.r_nm), "NM"
    assert np.array_equal(got.cigar_off, want.cig_off), "CIGAR lengths"
    assert np.array_equal(got.cigar, want.cig), "CIGAR"
    assert np.array_equal(got.md_off, want.md_off), "MD lengths"
    assert np.array_equal(got.md, want.md), "MD"
    assert np.array_equal(got.stats, want.stats)


def same_pairs(got, want):
    for k, v in want.items():
        if k == "n_proper":
            assert got.n_proper == v
        else:
            assert np.array_equal(getattr(got, k), v), k


def check_members(data, payload):
    members = bm.parse_bgzf(data, eof=False)
    assert gzip.decompress(data + bm.BGZF_EOF) == payload
    assert b"".join(m[0] for m in members) == payload
    for raw, size, _ in members:
        assert size <= 18 + 5 + len(raw) + 8, "a member larger than its stored form"
    return members


def bam_vs_sam(dev, slot, ref_names, n_sam=None):
    """fetch_sam and fetch_bam on the slot's staged batch: equal counters, level 0 == the model's encoding of the text, level 1
    inflates to it, no record spans two members, nowait gives the same bytes.  Returns the SAM text."""
    text, n_records, n_asserted, stats = dev.fetch_sam(slot=slot)
    want = bm.sam_to_bam_payload(text, ref_names)
    for level in (0, 1):
        data, raw_len, n_blocks, n_rec_b, n_ass_b, stats_b = dev.fetch_bam(slot=slot, level=level)
        assert (n_rec_b, n_ass_b) == (n_records, n_asserted) and np.array_equal(stats_b, stats)
        assert raw_len == len(want)
        members = check_members(data, want) if want else []
        assert data or not want
        assert len(members) == n_blocks
        if level == 0:
            assert all(m[2] == 0 for m in members)
        at = 0
        for raw, _, _ in members:  # whole records in every member, packed greedily
            bm.records(raw)
            at += len(raw)
            if at < len(want):
                nxt = struct.unpack_from("<i", want, at)[0] + 4
                assert len(raw) + nxt > bm.MEMBER_INPUT
        again = dev.fetch_bam(slot=slot, level=level, nowait=True)
        assert again[0] == data
    if n_sam is not None:
        assert bm.bam_payload_to_sam(want, ref_names) == text
    return text


def decode_bam_file(path):
    raw = b"".join(m[0] for m in bm.parse_bgzf(open(path, "rb").read()))
    assert raw[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", raw, 4)
    text = raw[8:8 + l_text]
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", raw, p)
    p += 4
    names = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, p)
        names.append(raw[p + 4:p + 4 + ln - 1])
        p += 8 + ln
    return text + bm.bam_payload_to_sam(raw[p:], names)


def pairing_on(dev, I, X, E):
    """Pairing within (I, X) with both kinds of rescue up to E edits, MAPQ and the unmapped reads' lines, on slot 0."""
    dev.set_pairs(I, X)
    dev.set_rescue(E)
    dev.set_rescue_discordant(True)
    dev.set_mapq(True)
    dev.set_unmapped(True)


def set_line_filter(dev, slot, mapq, unmapped, strata, max_hits):
    dev.set_mapq(mapq, slot=slot)
    dev.set_unmapped(unmapped, slot=slot)
    dev.set_report(strata, max_hits, slot=slot)


# ---- references the library takes for dense: synthetic ones large enough, banks, the forms of the join's table ----

def dense_setup(seed, seq_lens):
    from fem_amd import Device, host
    for k in ("FEM_FORCE_GENERIC", "FEM_FORCE_HASH", "FEM_FORCE_DENSE", "FEM_NO_DENSE", "FEM_TEST_TINY_BUFFERS"):
        assert os.environ.get(k, "0") == "0", k
    text, off, lens = host.synth_reference(seed, seq_lens, threads=8)
    seqs = [text[int(o):int(o) + int(l)] for o, l in zip(off, lens)]
    ref = fo.Reference([s.tobytes() for s in seqs])
    idx = fo.OracleIndex(ref)
    dev = Device(0)
    dev.upload_reference(seqs)
    n, lookup, occ = dev.build_index(12, 3)  # also checks the device index build at this size, byte for byte
    assert n == idx.n_occ and np.array_equal(lookup, idx.lookup) and np.array_equal(occ, idx.occ[:n])
    return dict(text=text, off=off, lens=lens, ref=ref, idx=idx, dev=dev)


def banked_device(bank_bases, bank_seqs=None):
    env = dict(FEM_FORCE_DENSE=1, FEM_TEST_BANK_BASES=bank_bases)
    if bank_seqs:
        env["FEM_TEST_BANK_SEQS"] = bank_seqs
    return device_with_env(**env)


def banked_compare(dev, seqs, reads, e, a, banked=True):
    ref = fo.Reference(seqs)
    idx = fo.OracleIndex(ref)
    batch = fo.ReadBatch(reads)
    want = fo.map_reads(ref, idx, batch, e=e, a=a)
    dev.upload_reference(seqs)
    dev.upload_index(12, 3, idx.lookup, idx.occ[:idx.n_occ])
    assert dev.seed_kernel(e=e, a=a) == ("seed_join_banked_kernel" if banked else "seed_join_kernel")
    got = dev.map_batch(batch.bases, batch.off, e=e, a=a)
    assert_same(want, got)
    rec = dev.fetch_records()  # the tail works on (sequence, position): nothing of the banks is left in it
    assert np.array_equal(rec.rec_begin, want.rec_off) and np.array_equal(rec.tid, want.r_tid) and np.array_equal(rec.pos0, want.r_pos)
    assert np.array_equal(rec.cigar, want.cig) and np.array_equal(rec.md, want.md)
    return want


JOIN_FORMS = {"padded": {}, "compact": {"FEM_NO_STRIDED": "1"},
              "banked": {"FEM_TEST_BANK_BASES": "10000000", "FEM_TEST_BANK_SEQS": "2"}}


class JoinWorld:
    """One dense handle per form of the join's table (JOIN_FORMS) over a world's seqs and idx, opened when first asked for."""

    def device(self, form):
        if form not in self.devices:
            dev = device_with_env(FEM_FORCE_DENSE="1", **JOIN_FORMS[form])
            dev.upload_reference(self.seqs)
            dev.upload_index(12, 3, self.idx.lookup, self.idx.occ[:self.idx.n_occ])
            info = dev.index_info()
            assert ("strided with pads" in info) == (form == "padded"), info
            assert ("2 banks" in info) == (form == "banked"), info
            self.devices[form] = dev
        return self.devices[form]

    def close(self):
        for dev in self.devices.values():
            dev.close()


def join_check(w, form, batch, want, e, a):
    dev = w.device(form)
    assert dev.seed_kernel(e=e, a=a) == ("seed_join_banked_kernel" if form == "banked" else "seed_join_kernel")
    assert_same(want, dev.map_batch(batch.bases, batch.off, e=e, a=a))
