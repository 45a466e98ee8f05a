"""tools/adapter_measure.py [n_reads]: the device time of the trim stage with the adapter match in it (fem_dev_set_adapter) per million
reads, beside the fixed trims alone and the mapping's kernels.

Kernel times (timing on) of the trim stage (id 19: the adapter match, clip points, the scan of the kept lengths, the gather), the seed
selection (8), the join (0) and the verification (1) on n_reads (default 1 M) of C3's synthetic reads, staged as characters with
Illumina-like qualities (tests/bam_model.py's four bins), with fixed trims alone (5, 5, 0), with the adapter alone, with the adapter
behind the fixed trims and with the adapter in front of the quality trim (0, 0, 20); and what was cut.  The reads hold no adapter: the
match runs through every window of every read, its worst case.  One JSON line on stdout."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from fem_amd import Device, host  # noqa: E402

IDS = (19, 8, 0, 2, 1)
ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    w = bench.WORKLOADS["c3"]
    text, off, lens = host.synth_reference(3, w["seq_lens"], threads=16)
    dev = Device(0)
    dev.upload_reference([text[int(o):int(o) + int(ln)] for o, ln in zip(off, lens)])
    dev.build_index(12, 3, fetch=False)
    bases, _ = host.synth_reads(w["seed"], text, off, lens, n, w["L"], w["e"], first_read=0, threads=16)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(w["L"])
    rng = np.random.default_rng(1)
    quals = (33 + rng.choice([2, 12, 23, 37], size=n * w["L"], p=[0.03, 0.07, 0.15, 0.75])).astype(np.uint8)
    rnames = ["r%d" % i for i in range(n)]
    out = {"n_reads": n, "L": w["L"], "e": w["e"], "seed_kernel": dev.seed_kernel(e=w["e"])}
    for tag, trim, adapter in (("fixed_5_5", (5, 5, 0), None), ("adapter", (0, 0, 0), ADAPTER), ("adapter_fixed_5_5", (5, 5, 0), ADAPTER),
                               ("qual_20", (0, 0, 20), None), ("adapter_qual_20", (0, 0, 20), ADAPTER)):
        dev.set_trim(*trim)
        dev.set_adapter(adapter)
        r = {}
        for rep in range(2):  # (the first is the warm-up)
            dev.set_timing(rep == 1)
            dev.reset_timing()
            dev.stage_reads(bases, offs)
            dev.stage_text(quals, rnames)
            dev.map_staged(e=w["e"])
            stats = dev.fetch_stats()
            if rep == 1:
                r = {"kernel%d_ms_per_M" % k: round(dev.kernel_time(k)[0] * 1e6 / n, 4) for k in IDS if dev.kernel_time(k)[1]}
                r["mapped"], r["packed"] = int(stats[1]), bool(dev.stage_info()[1])
                r["trimmed_reads"], r["trimmed_bases"] = dev.trim_count()
                r["adapter_reads"], r["adapter_bases"] = dev.adapter_count()
        dev.set_timing(False)
        out[tag] = r
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
