"""tools/paired_files.py <n_pairs> <dir>: the C3 reference (FASTA + index) and n_pairs read pairs (r1.fq, r2.fq) for
`FEM map --read2` runs, left in <dir>.

Fragments of 200..500 bp on the reference, mates of 100 bp: mate 1 the fragment's first bases, mate 2 the reverse complement of
its last, swapped in half the pairs.  Each mate carries 0..3 substitutions (e = 3); in 5 % of the pairs one mate carries 4..8
edits instead (60 % substitutions, 20 % insertions, 20 % deletions): single-end mapping at e = 3 misses it, --rescue 8 finds it."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fem_amd import host  # noqa: E402

L, E_HEAVY, HEAVY = 100, 8, 0.05
ACGT = np.frombuffer(b"ACGT", np.uint8)


def mates(text, off, lens, n):
    """The n pairs' mates on the reference (text, off, lens of host.synth_reference): two (n, L) uint8 arrays."""
    rng = np.random.default_rng(17)
    lens64 = lens.astype(np.int64)
    seq = rng.choice(len(lens64), size=n, p=lens64 / lens64.sum())
    frag = rng.integers(200, 501, size=n)
    st = off.astype(np.int64)[seq] + (rng.random(n) * (lens64[seq] - 520)).astype(np.int64)
    cols = np.arange(L)
    m1 = text[st[:, None] + cols]
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    m2 = comp[text[(st + frag - L)[:, None] + cols]][:, ::-1]
    for m in (m1, m2):  # 0..3 substitutions
        k = rng.integers(0, 4, size=n)
        for j in range(3):
            rows = np.nonzero(k > j)[0]
            at = rng.integers(0, L, size=len(rows))
            code = np.searchsorted(ACGT, m[rows, at])
            m[rows, at] = ACGT[(code + rng.integers(1, 4, size=len(rows))) % 4]
    for i in np.nonzero(rng.random(n) < HEAVY)[0]:  # one mate with 4..8 edits
        m = m1 if rng.random() < 0.5 else m2
        s = bytearray(m[i].tobytes())
        for _ in range(int(rng.integers(4, E_HEAVY + 1))):
            at, r = int(rng.integers(1, len(s) - 1)), rng.random()
            if r < 0.6:
                s[at] = int(ACGT[(np.searchsorted(ACGT, s[at]) + rng.integers(1, 4)) % 4])
            elif r < 0.8:
                s.insert(at, int(ACGT[rng.integers(0, 4)]))
            else:
                del s[at]
        s = (bytes(s) + bytes(ACGT[rng.integers(0, 4, size=L)]))[:L]
        m[i] = np.frombuffer(s, np.uint8)
    swap = rng.random(n) < 0.5
    m1[swap], m2[swap] = m2[swap].copy(), m1[swap].copy()
    return m1, m2


def main():
    n, d = int(sys.argv[1]), sys.argv[2]
    w = bench.WORKLOADS["c3"]
    os.makedirs(d, exist_ok=True)
    text, off, lens = host.synth_reference(3, w["seq_lens"], threads=16)
    fa, ix = os.path.join(d, "ref.fa"), os.path.join(d, "ref.idx")
    host.write_fasta(fa, text, off, lens)
    m1, m2 = mates(text, off, lens, n)
    for name, m in (("r1.fq", m1), ("r2.fq", m2)):
        bases = np.zeros(n * L + 8, np.uint8)
        bases[:n * L] = m.reshape(-1)
        host.write_fastq(os.path.join(d, name), bases, L, n)
    r = subprocess.run([os.path.join(ROOT, "fem_amd", "csrc", "FEM"), "index", "12", "3", fa, ix], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-300:]
    print("files in", d, "pairs", n)


if __name__ == "__main__":
    main()
