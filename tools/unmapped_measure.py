"""tools/unmapped_measure.py [n_reads]            the cost of --unmapped on the device, per 1 M reads
tools/unmapped_measure.py files <n_reads> <dir>  <dir>/mixed.fq: C3's reads with every fourth one replaced by random letters

Kernel times (timing on) of the line index (id 14), the SAM text kernels (id 7), the BAM record kernels (id 11) and
pair_kernel (id 9), with the switch off and on, and the bytes of SAM text, on three inputs of n_reads (default 1 M): C3's
synthetic reads (nearly all map: the price of the line index alone), the same with a quarter of random-letter reads, and
n_reads / 2 pairs of tools/paired_files.py.  One JSON line on stdout."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from fem_amd import Device, host  # noqa: E402
sys.path.insert(0, os.path.join(os.getcwd(), "tools"))
import paired_files  # noqa: E402

SHARE = 4  # every fourth read of the mixed input is random letters
w = bench.WORKLOADS["c3"]


def mixed(bases, n):
    rows = np.array(bases[:n * w["L"]]).reshape(n, w["L"])
    rng = np.random.default_rng(29)
    k = len(rows[::SHARE])
    rows[::SHARE] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(k, w["L"]))]
    return np.concatenate([rows.reshape(-1), np.zeros(8, np.uint8)])


def main_files():
    n, d = int(sys.argv[2]), sys.argv[3]
    text, off, lens = host.synth_reference(3, w["seq_lens"], threads=16)
    bases, _ = host.synth_reads(w["seed"], text, off, lens, n, w["L"], w["e"], first_read=0, threads=16)
    host.write_fastq(os.path.join(d, "mixed.fq"), mixed(bases, n), w["L"], n)
    print("mixed.fq in", d, "reads", n, "of random letters", (n + SHARE - 1) // SHARE)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    text, off, lens = host.synth_reference(3, w["seq_lens"], threads=16)
    dev = Device(0)
    dev.upload_reference([text[int(o):int(o) + int(ln)] for o, ln in zip(off, lens)])
    dev.upload_reference_names(["chr%d" % (i + 1) for i in range(len(lens))])
    dev.build_index(12, 3, fetch=False)
    se_bases, se_offs = host.synth_reads(w["seed"], text, off, lens, n, w["L"], w["e"], first_read=0, threads=16)
    m1, m2 = paired_files.mates(text, off, lens, n // 2)
    pe_bases = np.concatenate([m1.reshape(-1), m2.reshape(-1), np.zeros(8, np.uint8)])
    rnames = ["SRR0000001.%d" % (i + 1) for i in range(n)]
    dev.reserve_batch(n, n + n // 4, w["L"], e=w["e"])
    out = {"workload": "c3", "n_reads": n, "e": w["e"], "pairs": n // 2, "random_share": 1.0 / SHARE}

    def timed(bases, offs, bam):
        quals = np.full(len(bases), ord("I"), np.uint8)

        def staged():
            dev.stage_reads(bases, offs)
            dev.stage_text(quals, rnames[:len(offs) - 1])
            dev.map_staged(e=w["e"])

        staged()
        dev.fetch_bam(level=0) if bam else dev.fetch_sam()  # (warm)
        staged()
        dev.set_timing(True)
        dev.reset_timing()
        got = dev.fetch_bam(level=0) if bam else dev.fetch_sam()
        r = {"kernel%d_ms_per_M" % k: dev.kernel_time(k)[0] * 1e6 / n for k in (9, 14, 11 if bam else 7) if dev.kernel_time(k)[1]}
        r["bytes"] = int(got[1]) if bam else len(got[0])
        r["mapped_reads"] = int(got[-1][1])
        dev.set_timing(False)
        return r

    inputs = (("c3", se_bases, False), ("mixed", mixed(se_bases, n), False), ("pairs", pe_bases, True))
    for name, bases, pairs in inputs:
        offs = np.arange((len(bases) - 8) // w["L"] + 1, dtype=np.uint64) * np.uint64(w["L"])
        dev.set_pairs(0, 500) if pairs else dev.set_pairs(None)
        for on in (False, True):
            dev.set_unmapped(on)
            for bam in (False, True):
                r = timed(bases, offs, bam)
                r["unmapped_lines"] = dev.unmapped_count()
                out["%s_%s_%s" % (name, "bam" if bam else "sam", "on" if on else "off")] = r
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main_files() if len(sys.argv) > 1 and sys.argv[1] == "files" else main()
