"""tools/xa_measure.py [n_reads]: what folding secondary lines into XA:Z (fem_dev_set_xa) costs and buys on the device, per 1 M reads.

Kernel times (timing on) of the fold index (id 18), the line filter's index (id 15), the SAM text kernels (id 7) and the BAM record
kernels (id 11), and the bytes of SAM text and of BAM records, with the option off and on (no entry limit), on three inputs of n_reads
(default 1 M): C3's synthetic reads (about one line per read: the price of the index alone), a quarter as many reads on the repeat-rich c3r
reference (tens of lines per read: what folding saves), and n_reads / 2 pairs of tools/paired_files.py with rescue at 8 edits.
FEM_HIP_LIBRARY names another build of the library (one without the option measures its "off" alone).  One JSON line on stdout."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from fem_amd import Device, host  # noqa: E402
sys.path.insert(0, os.path.join(os.getcwd(), "tools"))
import paired_files  # noqa: E402

IDS = (7, 11, 15, 18)


def reference(key):
    w = bench.WORKLOADS[key]
    text, off, lens = host.synth_reference(3, w["seq_lens"], threads=16)
    if "repeats" in w:
        bench.plant_repeats(text, off, lens, **w["repeats"])
    return w, text, off, lens


def measure(key, n, out, with_pairs):
    w, text, off, lens = reference(key)
    dev = Device(0)
    dev.upload_reference([text[int(o):int(o) + int(ln)] for o, ln in zip(off, lens)])
    dev.upload_reference_names(["chr%d" % (i + 1) for i in range(len(lens))])
    dev.build_index(12, 3, fetch=False)
    has_option = hasattr(dev._L, "fem_dev_set_xa")
    n_ids = [k for k in IDS if k < 18 or has_option]
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
        r = {"kernel%d_ms_per_M" % k: round(dev.kernel_time(k)[0] * 1e6 / n, 4) for k in n_ids if dev.kernel_time(k)[1]}
        r["bytes"] = int(got[1]) if bam else len(got[0])
        r["bytes_per_read"] = round(r["bytes"] / (len(offs) - 1), 1)
        r["records"] = int(got[3] if bam else got[1])
        if not bam:  # lines, and those that carry XA: entries per folding slot says whether the entry limit or the byte budget binds
            r["lines"], r["xa_lines"] = got[0].count(b"\n"), got[0].count(b"\tXA:Z:")
        dev.set_timing(False)
        return r

    for name, bases, pairs in inputs:
        offs = np.arange((len(bases) - 8) // w["L"] + 1, dtype=np.uint64) * np.uint64(w["L"])
        dev.set_pairs(0, 500) if pairs else dev.set_pairs(None)
        dev.set_rescue(8 if pairs else None)
        for tag in ("off", "on") if has_option else ("off",):
            if has_option:
                dev.set_xa(Device.XA_ALL if tag == "on" else 0)
            for bam in (False, True):
                r = timed(bases, offs, bam)
                if has_option:
                    r["xa_entries"] = dev.xa_count()
                out["%s_%s_%s" % (name, "bam" if bam else "sam", tag)] = r
    dev.close()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    out = {"library": os.environ.get("FEM_HIP_LIBRARY", "this build"), "n_reads": n, "e": bench.WORKLOADS["c3"]["e"], "pairs": n // 2, "rescue": 8, "c3r_reads": n // 4}
    measure("c3", n, out, True)
    measure("c3r", n // 4, out, False)  # (tens of lines per read: a quarter of the reads keeps the unfolded text under 2 GB)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
