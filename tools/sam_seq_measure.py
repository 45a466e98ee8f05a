"""tools/sam_seq_measure.py [n_reads] [reps]: the device time of the text stage on one batch of C2's reads (100 bases, e = 3; about half
the mapped reads on the reverse strand) — the SAM text kernels (id 7) and the BAM record kernels (id 11), per repetition, with
fem_dev_set_sam_seq off and, where the library has it, on.  FEM_HIP_LIBRARY names another build of the library (the build a change
is compared against).  A warm-up fetch of each kind first.  One JSON line on stdout."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from fem_amd import Device, host  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 250_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
w = bench.WORKLOADS["c2"]
text, off, lens = host.synth_reference(w["seed"], w["seq_lens"], threads=16)
dev = Device(0)
dev.upload_reference([text[int(o):int(o) + int(ln)] for o, ln in zip(off, lens)])
dev.upload_reference_names(["chr%d" % (i + 1) for i in range(len(lens))])
dev.build_index(12, 3, fetch=False)
bases, offs = host.synth_reads(w["seed"], text, off, lens, n, w["L"], w["e"], first_read=0, threads=16)
quals = (33 + np.arange(len(bases), dtype=np.uint32) % 41).astype(np.uint8)
rnames = ["SRR0000001.%d" % (i + 1) for i in range(n)]
dev.reserve_batch(n, n + n // 4, w["L"], e=w["e"])
has_option = hasattr(dev._L, "fem_dev_set_sam_seq")
out = {"library": os.environ.get("FEM_HIP_LIBRARY", "this build"), "workload": "c2", "n_reads": n, "e": w["e"], "reps": reps}


def batch():
    dev.stage_reads(bases, offs)
    dev.stage_text(quals, rnames)
    dev.map_staged(e=w["e"])


def timed():
    sam, bam = [], []
    batch()
    text_bytes = len(dev.fetch_sam()[0])  # (warm)
    dev.fetch_bam(level=0)
    for _ in range(reps):
        batch()
        dev.set_timing(True)
        dev.reset_timing()
        dev.fetch_sam()
        sam.append(round(dev.kernel_time(7)[0], 4))
        dev.reset_timing()
        dev.fetch_bam(level=0)
        bam.append(round(dev.kernel_time(11)[0], 4))
        dev.set_timing(False)
    return {"sam_ms": sam, "bam_ms": bam, "text_bytes": text_bytes}


out["off"] = timed()
if has_option:
    dev.set_sam_seq(True)
    out["on"] = timed()
    lines = dev.fetch_sam()[0].splitlines()
    out["lines"], out["turned"] = len(lines), sum(1 for l in lines if int(l.split(b"\t", 2)[1]) & 16 and l.split(b"\t")[9] != b"*")
dev.close()
print(json.dumps(out))
