"""tools/report_measure.py [n_reads]                 the cost and the gain of the line filter on the device, per 1 M reads
tools/report_measure.py files <n_reads> <dir>     <dir>: ref.fa, ref.idx and reads.fq of the repeat-rich c3r workload

Kernel times (timing on) of the filter's line index (id 15), the SAM text kernels (id 7) and the BAM record kernels (id 11)
and the bytes of SAM text and of BAM records, with the filter off, with max_hits = 1 and with strata = 0, on three inputs of
n_reads (default 1 M): C3's synthetic reads (about one line per read: the price of the line index alone), the same reads on
the repeat-rich c3r reference (tens of lines per read: what the filter saves), and n_reads / 2 pairs of
tools/paired_files.py with rescue at 8 edits.  One JSON line on stdout."""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from fem_amd import Device, host  # noqa: E402
sys.path.insert(0, os.path.join(os.getcwd(), "tools"))
import paired_files  # noqa: E402

FILTERS = (("off", None, None), ("max_hits_1", None, 1), ("strata_0", 0, None))


def reference(key):
    w = bench.WORKLOADS[key]
    text, off, lens = host.synth_reference(3, w["seq_lens"], threads=16)
    if "repeats" in w:
        bench.plant_repeats(text, off, lens, **w["repeats"])
    return w, text, off, lens


def main_files():
    n, d = int(sys.argv[2]), sys.argv[3]
    os.makedirs(d, exist_ok=True)
    w, text, off, lens = reference("c3r")
    fa, fq, ix = (os.path.join(d, x) for x in ("ref.fa", "reads.fq", "ref.idx"))
    host.write_fasta(fa, text, off, lens)
    bases, _ = host.synth_reads(w["seed"], text, off, lens, n, w["L"], w["e"], first_read=0, threads=16)
    host.write_fastq(fq, bases, w["L"], n)
    r = subprocess.run([os.path.join(os.getcwd(), "fem_amd", "csrc", "FEM"), "index", "12", "3", fa, ix], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-300:]
    print("c3r files in", d, "reads", n)


def measure(key, n, out, with_pairs):
    w, text, off, lens = reference(key)
    dev = Device(0)
    dev.upload_reference([text[int(o):int(o) + int(ln)] for o, ln in zip(off, lens)])
    dev.upload_reference_names(["chr%d" % (i + 1) for i in range(len(lens))])
    dev.build_index(12, 3, fetch=False)
    se_bases, _ = host.synth_reads(w["seed"], text, off, lens, n, w["L"], w["e"], first_read=0, threads=16)
    inputs = [(key, se_bases, False)]
    if with_pairs:
        m1, m2 = paired_files.mates(text, off, lens, n // 2)
        inputs.append(("pairs", np.concatenate([m1.reshape(-1), m2.reshape(-1), np.zeros(8, np.uint8)]), True))
    rnames = ["SRR0000001.%d" % (i + 1) for i in range(n)]

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
        r = {"kernel%d_ms_per_M" % k: dev.kernel_time(k)[0] * 1e6 / n for k in (15, 11 if bam else 7) if dev.kernel_time(k)[1]}
        r["bytes"] = int(got[1]) if bam else len(got[0])
        r["records"] = int(got[3] if bam else got[1])
        dev.set_timing(False)
        return r

    for name, bases, pairs in inputs:
        offs = np.arange((len(bases) - 8) // w["L"] + 1, dtype=np.uint64) * np.uint64(w["L"])
        dev.set_pairs(0, 500) if pairs else dev.set_pairs(None)
        dev.set_rescue(8 if pairs else None)
        for tag, strata, max_hits in FILTERS:
            dev.set_report(strata, max_hits)
            for bam in (False, True):
                r = timed(bases, offs, bam)
                r["filtered_lines"] = dev.filtered_count()
                out["%s_%s_%s" % (name, "bam" if bam else "sam", tag)] = r
    dev.close()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    out = {"n_reads": n, "e": bench.WORKLOADS["c3"]["e"], "pairs": n // 2, "rescue": 8}
    measure("c3", n, out, True)
    measure("c3r", n, out, False)
    print(json.dumps(out))


if __name__ == "__main__":
    main_files() if len(sys.argv) > 1 and sys.argv[1] == "files" else main()
