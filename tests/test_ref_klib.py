"""libfemhost's sequence readers and the mapping sort against THE REFERENCE'S OWN klib code: oracle/_ref/libfemref_klib.so
is the reference's src/kseq.h and src/ksort.h, compiled from where they lie in the reference's tree behind the harness
oracle/ref_klib.c (`make -C oracle ref`; the rest of the reference, built against a stand-in for htslib: tests/test_ref_parity.py).

  * records: kseq_read as src/sequence_batch.c:47-66 drives it (zero-length records skipped, any return below -1 fatal)
    vs fem_seqfile_read (sequential), fem_seqfile_read_bytes and fem_seqfile_plan/_fill (multi-threaded), plain and gzip
  * order of a read's mappings: radix_sort_mapping (src/align.c:53-57) vs the oracle's restatement, which the host tail
    and the device ordering kernel are compared with elsewhere (tests/test_host.py, tests/test_gpu_tail.py)

Without the library (a checkout that never saw the reference's sources) what it returned stands in:
tests/golden/klib_records.npz holds, for every input these tests give it (keyed by a hash of the input), SHA-1
fingerprints of what they compare: the loader's view of a file's records, the sort's permutation.  The vectors of
tests/golden/klib_kseq.npz and klib_sort.npz are compared in full.  All are made by tests/golden/make_klib_golden.py."""
import gzip
import os

import numpy as np
import pytest

from fem_amd import host
from oracle import fem_oracle as fo
from oracle import ref_klib
from tests.cases import HAND_MADE, StoredView, file_key, input_key, loader_view, perm_fingerprint, random_file, sort_cases, view_fingerprints

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDS = os.path.join(GOLDEN, "klib_records.npz")
_stored = {}


def stored():
    """{"kseq": {key: (StoredView, last_rc)}, "sort": {key: fingerprint of perm}} (format: make_klib_golden.py)."""
    if not _stored:
        g = np.load(RECORDS)
        _stored["kseq"] = {k.tobytes(): (StoredView(int(n), bool(aq), ns.tobytes(), q.tobytes()), int(rc))
                           for k, n, aq, ns, q, rc in zip(g["kseq_key"], g["n_records"], g["all_qual"], g["names_seqs"],
                                                          g["quals"], g["last_rc"])}
        _stored["sort"] = {k.tobytes(): f.tobytes() for k, f in zip(g["sort_key"], g["perm"])}
    return _stored


def ref_view(path):
    """(loader's view of the reference's kseq_read records, fatal): live from oracle/_ref where it is built, else what it
    returned for the same input (a StoredView)."""
    if ref_klib.available():
        return loader_view(*ref_klib.kseq_records(path))
    got = stored()["kseq"].get(file_key(path))
    assert got is not None, "no stored kseq result for %s: tests/golden/make_klib_golden.py makes them" % path
    return got[0], got[1] != -1


def same_sort(keys, got_k, got_perm):
    """The oracle's sort of `keys` against the reference's radix_sort_mapping, live or by its stored permutation."""
    if ref_klib.available():
        want_k, want_perm = ref_klib.radix_sort(keys)
        assert np.array_equal(want_k, got_k)
        assert np.array_equal(want_perm, got_perm), "order among equal keys"
        return
    want = stored()["sort"].get(input_key(b"sort", np.ascontiguousarray(keys, dtype=np.uint64).tobytes()))
    assert want is not None, "no stored radix sort result for these %d keys" % len(keys)
    assert np.array_equal(keys[got_perm.astype(np.int64)], got_k)
    assert perm_fingerprint(got_perm) == want, "order among equal keys"


def ours_sequential(path):
    try:
        s = host.read_sequences(path)
    except ValueError:
        return None, True
    return [(s.name(i).encode(), s.seq(i), s.qual(i) if s.quals is not None else None) for i in range(s.n)], False


def ours_planned(path, approx, threads):
    try:
        parts = host.read_planned_batches(path, approx, threads=threads)
    except ValueError:
        return None, True
    out = []
    for p in parts:
        out += [(p.name(i).encode(), p.seq(i), p.qual(i) if p.quals is not None else None) for i in range(p.n)]
    return out, False


def same_records(ref, mine, quals=True):
    # (a batch keeps its qualities only if every record has them, fem_host.cc finish_seqset: they are compared then only)
    assert len(ref) == len(mine)
    if isinstance(ref, StoredView):
        names_seqs, q = view_fingerprints(mine)
        assert names_seqs == ref.names_seqs
        if quals and ref.all_qual and ref.n:
            assert q == ref.quals
        return
    all_qual = all(r[3] is not None for r in ref)
    for (name, _comment, seq, qual), (n2, s2, q2) in zip(ref, mine):
        assert name == n2 and seq == s2
        if quals and all_qual and ref:
            assert qual == q2


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_readers_follow_kseq_on_hand_made_files(tmp_path, name):
    data = HAND_MADE[name]
    for gz in (False, True):
        p = str(tmp_path / (name + (".fq.gz" if gz else ".fq")))
        with (gzip.open(p, "wb") if gz else open(p, "wb")) as f:
            f.write(data)
        ref, fatal = ref_view(p)
        mine, failed = ours_sequential(p)
        assert failed == fatal, name
        if not fatal:
            same_records(ref, mine)
        for approx, threads in ((0, 1), (64, 3)):
            mine, failed = ours_planned(p, approx, threads)
            assert failed == fatal, (name, approx)
            if not fatal:
                same_records(ref, mine)


def test_readers_follow_kseq_on_random_damaged_files(tmp_path):
    rng = np.random.default_rng(2024)
    n_fatal = n_ok = 0
    for case in range(1500):
        data = random_file(rng)
        p = str(tmp_path / ("f%d.fq" % case))
        with open(p, "wb") as f:
            f.write(data)
        ref, fatal = ref_view(p)
        mine, failed = ours_sequential(p)
        assert failed == fatal, (case, data)
        if not fatal:
            same_records(ref, mine)
        mine, failed = ours_planned(p, int(rng.choice([0, 50, 300])), int(rng.integers(1, 5)))
        assert failed == fatal, (case, data)
        if not fatal:
            same_records(ref, mine)
        n_fatal += fatal
        n_ok += not fatal
    assert n_fatal > 300 and n_ok > 300


def _oracle_sort(keys):
    k = keys.copy()
    perm = np.zeros(len(k), np.uint32)
    fo.lib().fo_sort_mapping_keys(k.ctypes.data, perm.ctypes.data, len(k))
    return k, perm


def test_mapping_order_follows_the_reference_radix_sort():
    n_tied = 0
    for keys in sort_cases():
        got_k, got_perm = _oracle_sort(keys)
        same_sort(keys, got_k, got_perm)
        n_tied += len(keys) - len(np.unique(keys))
    assert n_tied > 5000


def test_golden_vectors_made_from_the_reference_klib(tmp_path):
    """The same two comparisons against vectors committed under tests/golden/ (made by make_klib_golden.py from
    oracle/_ref): they hold wherever the tests run, with or without the reference."""
    g = np.load(os.path.join(GOLDEN, "klib_sort.npz"))
    for i in range(int(g["n_cases"])):
        keys, perm = g["keys_%d" % i], g["perm_%d" % i]
        got_k, got_perm = _oracle_sort(keys)
        assert np.array_equal(got_perm, perm) and np.array_equal(got_k, keys[perm])
    g = np.load(os.path.join(GOLDEN, "klib_kseq.npz"), allow_pickle=False)
    for i in range(int(g["n_cases"])):
        data = g["file_%d" % i].tobytes()
        p = str(tmp_path / ("g%d.fq" % i))
        with open(p, "wb") as f:
            f.write(data)
        fatal = bool(g["fatal_%d" % i])
        mine, failed = ours_sequential(p)
        assert failed == fatal
        if fatal:
            continue
        names = g["names_%d" % i].tobytes().split(b"\x00")[:-1] if g["names_%d" % i].size else []
        seqs = g["seqs_%d" % i].tobytes().split(b"\x00")[:-1] if g["seqs_%d" % i].size else []
        assert [m[0] for m in mine] == names and [m[1] for m in mine] == seqs
        planned, failed = ours_planned(p, 64, 2)
        assert not failed and [m[1] for m in planned] == seqs


def _random_fasta(rng):
    """Multi-line FASTA as references come, plus what kseq tolerates or reacts to: blank lines, '>' inside lines, empty
    records, comments, junk in front, lines that begin with '@' or '+', a carriage return, no final newline."""
    out = [b"junk before\n"] if rng.random() < 0.1 else []
    for i in range(int(rng.integers(1, 12))):
        ln = int(rng.integers(0, 400))
        width = int(rng.integers(5, 80))
        seq = bytes(rng.choice(list(b"ACGTNacgtn>"), size=ln, p=[.2, .2, .2, .2, .05, .03, .03, .03, .03, .02, .01]).astype(np.uint8))
        lines = [seq[j:j + width] for j in range(0, ln, width)]
        if rng.random() < 0.15:
            lines.insert(int(rng.integers(0, len(lines) + 1)), b"")  # blank line
        quirk = rng.random()
        if quirk < 0.03 and lines:
            lines[int(rng.integers(0, len(lines)))] = b"@odd"
        elif quirk < 0.06 and lines:
            lines[int(rng.integers(0, len(lines)))] = b"+odd"
        elif quirk < 0.09 and lines:
            lines[int(rng.integers(0, len(lines)))] += b"\r"
        name = b"s%d" % i + (b"\tdesc %d" % i if rng.random() < 0.4 else b"")
        out.append(b">" + name + b"\n" + b"".join(l + b"\n" for l in lines))
    data = b"".join(out)
    return data[:-1] if rng.random() < 0.2 and data.endswith(b"\n") else data


def test_parallel_fasta_reader_follows_kseq(tmp_path, monkeypatch):
    # fem_seqfile_read on a plain FASTA file is read_fasta_parallel (fem_host.cc) when the file is regular enough, the
    # sequential reader otherwise: either way kseq's records.  Small pieces so that every body is cut many times.
    rng = np.random.default_rng(31)
    n_multi = 0
    for case in range(600):
        monkeypatch.setenv("FEM_FASTA_PIECE", str(int(rng.choice([16, 40, 200, 100000]))))
        data = _random_fasta(rng)
        p = str(tmp_path / ("r%d.fa" % case))
        with open(p, "wb") as f:
            f.write(data)
        ref, fatal = ref_view(p)
        mine, failed = ours_sequential(p)
        assert failed == fatal, (case, data)
        if not fatal:
            assert len(ref) == len(mine), (case, data)
            same_records(ref, mine, quals=False)
            n_multi += len(ref) > 1
    assert n_multi > 300
