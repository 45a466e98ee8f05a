"""Makes tests/golden/klib_sort.npz, klib_kseq.npz and klib_records.npz from the reference's own klib code
(oracle/_ref/libfemref_klib.so = the reference's src/kseq.h + ksort.h behind oracle/ref_klib.c).  Run where the
reference's sources are (`make -C oracle ref` builds the library from REF):

    make -C oracle ref && python tests/golden/make_klib_golden.py

The vectors are inputs + what the reference code returned for them; no reference source is stored.  klib_records.npz
holds, for every input tests/test_ref_klib.py gives the reference, fingerprints of what those tests compare, recorded
while they run against the library (tests/cases.py: input_key / file_key / StoredView / perm_fingerprint):
    kseq_key[F, 8], last_rc[F], n_records[F], all_qual[F], names_seqs[F, 16], quals[F, 16]   per file
    sort_key[S, 8], perm[S, 16]                                                               per key array sorted"""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_klib  # noqa: E402
from tests import cases as T  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    out = {}
    cases = [k for k in T.sort_cases() if len(k) <= 1000]
    for i, keys in enumerate(cases):
        _, perm = ref_klib.radix_sort(keys)
        out["keys_%d" % i], out["perm_%d" % i] = keys, perm
    out["n_cases"] = np.int64(len(cases))
    np.savez_compressed(os.path.join(HERE, "klib_sort.npz"), **out)

    out = {}
    rng = np.random.default_rng(4)
    files = [T.HAND_MADE[k] for k in sorted(T.HAND_MADE)] + [T.random_file(rng) for _ in range(60)]
    with tempfile.TemporaryDirectory() as d:
        for i, data in enumerate(files):
            p = os.path.join(d, "f.fq")
            with open(p, "wb") as f:
                f.write(data)
            recs, fatal = T.loader_view(*ref_klib.kseq_records(p))
            out["file_%d" % i] = np.frombuffer(data, np.uint8)
            out["fatal_%d" % i] = np.bool_(fatal)
            out["names_%d" % i] = np.frombuffer(b"".join(r[0] + b"\x00" for r in recs), np.uint8)
            out["seqs_%d" % i] = np.frombuffer(b"".join(r[2] + b"\x00" for r in recs), np.uint8)
    out["n_cases"] = np.int64(len(files))
    np.savez_compressed(os.path.join(HERE, "klib_kseq.npz"), **out)
    print("wrote klib_sort.npz (%d cases) and klib_kseq.npz (%d files)" % (len(cases), len(files)))
    record()


def record():
    """Runs the tests of test_ref_klib.py that call the reference, with the library's two calls recorded."""
    kseq, sort = {}, {}
    live_kseq, live_sort = ref_klib.kseq_records, ref_klib.radix_sort

    def kseq_records(path):
        got = live_kseq(path)
        kseq[T.file_key(path)] = (T.StoredView.of(T.loader_view(*got)[0]), got[1])
        return got

    def radix_sort(keys):
        got = live_sort(keys)
        sort[T.input_key(b"sort", np.ascontiguousarray(keys, dtype=np.uint64).tobytes())] = T.perm_fingerprint(got[1])
        return got

    ref_klib.kseq_records, ref_klib.radix_sort = kseq_records, radix_sort
    try:
        rc = pytest.main(["-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_ref_klib.py"), "-k", "follow"])
    finally:
        ref_klib.kseq_records, ref_klib.radix_sort = live_kseq, live_sort
    if rc != 0:
        raise SystemExit("tests/test_ref_klib.py failed against the library (%s): nothing written" % rc)

    def rows(values):
        return np.array([np.frombuffer(v, np.uint8) for v in values], np.uint8).reshape(len(values), -1)
    views = [v for v, _ in kseq.values()]
    np.savez_compressed(os.path.join(HERE, "klib_records.npz"),
                        kseq_key=rows(list(kseq)), last_rc=np.array([rc_ for _, rc_ in kseq.values()], np.int32),
                        n_records=np.array([v.n for v in views], np.uint32), all_qual=np.array([v.all_qual for v in views], np.uint8),
                        names_seqs=rows([v.names_seqs for v in views]), quals=rows([v.quals for v in views]),
                        sort_key=rows(list(sort)), perm=rows(list(sort.values())))
    print("wrote klib_records.npz (%d files, %d sorts)" % (len(kseq), len(sort)))


if __name__ == "__main__":
    main()
