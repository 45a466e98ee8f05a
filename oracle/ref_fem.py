"""ctypes binding of oracle/_ref/libfemref_fn.so (the reference's own functions behind oracle/ref_fn.c) and a runner for
oracle/_ref/FEM_ref (the reference's command line).  TEST INFRASTRUCTURE ONLY: loaded by tests/ and
tests/golden/make_ref_golden.py, never by the product.  Both are built by `make -C oracle ref` where the reference's
sources exist, against the htslib stand-in (oracle/ref_standin/), and ship to the GPU box as built."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

COUNTER_LABELS = ["The number of read", "The number of mapped read",
                  "The number of candidate before additional q-gram filter", "The number of candidate",
                  "The number of mapping"]  # src/FEM_map.c:214-218, the order of MappingStats


def lib_path():
    return os.path.join(_HERE, "_ref", "libfemref_fn.so")


def cli_path():
    return os.path.join(_HERE, "_ref", "FEM_ref")


def available():
    return os.path.exists(lib_path()) and os.path.exists(cli_path())


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(lib_path())
        vp = C.c_void_p
        L.rf_open.restype = vp
        L.rf_open.argtypes = [C.c_char_p]
        L.rf_close.argtypes = [vp]
        L.rf_num_sequences.restype = C.c_uint32
        L.rf_num_sequences.argtypes = [vp]
        L.rf_sequence_length.restype = C.c_uint32
        L.rf_sequence_length.argtypes = [vp, C.c_uint32]
        L.rf_sequence_name.restype = C.c_char_p
        L.rf_sequence_name.argtypes = [vp, C.c_uint32]
        L.rf_index_construct.argtypes = [vp, C.c_int, C.c_int]
        L.rf_index_save.argtypes = [vp, C.c_char_p]
        L.rf_index_load.argtypes = [vp, C.c_char_p]
        L.rf_index_arrays.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(vp), C.POINTER(C.c_uint64),
                                      C.POINTER(vp)]
        L.rf_load_reads.restype = C.c_uint32
        L.rf_load_reads.argtypes = [vp, C.c_char_p, C.c_uint32]
        L.rf_read_length.restype = C.c_uint32
        L.rf_read_length.argtypes = [vp, C.c_uint32]
        L.rf_candidates.restype = C.c_uint32
        L.rf_candidates.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, C.c_uint32, C.POINTER(C.c_uint32)]
        L.rf_verify.restype = C.c_uint32
        L.rf_verify.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, vp, C.c_uint32, vp, vp, vp, vp]
        L.rf_align.restype = C.c_int
        L.rf_align.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, C.c_uint64, C.c_int, C.c_int, vp, C.c_int,
                               C.POINTER(C.c_int), C.c_char_p, C.c_int]
        _LIB = L
    return _LIB


class RefFem:
    """The reference's functions on one reference file and (after load_reads) one batch of reads."""

    def __init__(self, reference_path):
        self._L = lib()
        self._h = C.c_void_p(self._L.rf_open(reference_path.encode()))
        self.n_reads = 0

    def close(self):
        if self._h:
            self._L.rf_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sequences(self):
        """[(name, length), ...] as the reference's loader saw them."""
        n = self._L.rf_num_sequences(self._h)
        return [(self._L.rf_sequence_name(self._h, i).decode(), int(self._L.rf_sequence_length(self._h, i)))
                for i in range(n)]

    def construct_index(self, k, step):
        self._L.rf_index_construct(self._h, k, step)

    def save_index(self, path):
        self._L.rf_index_save(self._h, path.encode())

    def load_index(self, path):
        self._L.rf_index_load(self._h, path.encode())

    def index_arrays(self):
        """(k, step, lookup, occ): copies of the resident index's tables."""
        k, step, n = C.c_int(), C.c_int(), C.c_uint64()
        lk, oc = C.c_void_p(), C.c_void_p()
        self._L.rf_index_arrays(self._h, C.byref(k), C.byref(step), C.byref(lk), C.byref(n), C.byref(oc))
        lookup = np.frombuffer(C.string_at(lk.value, 4 * ((1 << (2 * k.value)) + 1)), np.uint32).copy()
        occ = np.frombuffer(C.string_at(oc.value, 8 * n.value), np.uint64).copy() if n.value else np.zeros(0, np.uint64)
        return k.value, step.value, lookup, occ

    def load_reads(self, reads_path, max_reads):
        n = self._L.rf_load_reads(self._h, reads_path.encode(), max_reads)
        assert n != 0xFFFFFFFF, "one batch of reads per handle"
        self.n_reads = int(n)
        return self.n_reads

    def read_length(self, read):
        return int(self._L.rf_read_length(self._h, read))

    def candidates(self, e, a, read, direction):
        """(candidates of one strand, count before the additional q-gram filter)."""
        cap = 1 << 12
        while True:
            buf = np.zeros(cap, np.uint64)
            pre = C.c_uint32(0)
            n = self._L.rf_candidates(self._h, e, a, read, direction, buf.ctypes.data, cap, C.byref(pre))
            if n <= cap:
                return buf[:n].copy(), int(pre.value)
            cap = int(n)

    def verify(self, e, a, read, direction, candidates):
        """(ed, end, dir, cand) of the mappings verify_candidates appends for these candidates, in its order."""
        c = np.ascontiguousarray(candidates, dtype=np.uint64)
        n = len(c)
        ed, end = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int16)
        dr, cand = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64)
        m = self._L.rf_verify(self._h, e, a, read, direction, c.ctypes.data, n, ed.ctypes.data, end.ctypes.data,
                              dr.ctypes.data, cand.ctypes.data)
        return ed[:m], end[:m], dr[:m], cand[:m]

    def align(self, e, read, direction, candidate, ed, end):
        """(start offset in the candidate's window, CIGAR string, MD string) of generate_alignment."""
        L = self.read_length(read)
        cig = np.zeros(L + 2, np.uint32)
        n = C.c_int(0)
        md = C.create_string_buffer(16 * L + 64)
        start = self._L.rf_align(self._h, e, read, direction, int(candidate), int(ed), int(end), cig.ctypes.data, len(cig),
                                 C.byref(n), md, len(md))
        cigar = "".join("%d%s" % (int(o) >> 4, "MIDNSHP=X"[int(o) & 0xF]) for o in cig[:n.value])
        return start, cigar, md.value.decode()


def run_cli(*args, timeout=300):
    """FEM_ref with these arguments as a child process: CompletedProcess (returncode -6: an assert of the reference)."""
    return subprocess.run([cli_path()] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=timeout)


def cli_index(k, step, reference_path, index_path):
    r = run_cli("index", k, step, reference_path, index_path)
    assert r.returncode == 0, r.stderr.decode(errors="replace")


def cli_map(e, a, reference_path, index_path, reads_path, sam_path, threads=1):
    """FEM_ref map: (CompletedProcess, the five counters of its stderr or None where it did not finish)."""
    r = run_cli("map", "-e", e, "-a", a, "-t", threads, "--ref", reference_path, "--index", index_path, "--read1",
                reads_path, "-o", sam_path)
    return r, parse_counters(r.stderr.decode(errors="replace"))


def parse_counters(stderr_text):
    out = []
    for label in COUNTER_LABELS:
        hit = [l for l in stderr_text.splitlines() if l.startswith(label + ": ")]
        if len(hit) != 1:
            return None
        out.append(int(hit[0].rsplit(": ", 1)[1]))
    return np.array(out, dtype=np.uint64)
