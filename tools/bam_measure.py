"""tools/bam_measure.py [n_reads]: BAM output on C3 — the device time of the BAM record kernels (id 11) and the BGZF kernels
(id 12) per 1 M reads, and compressed bytes per read: C3's synthetic reads (constant 'I' qualities, a flattering ratio), and
payloads with Illumina-like 4-bin and unbinned random-walk qualities.  One JSON line on stdout."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from fem_amd import Device, host  # noqa: E402
from tests import bam_model as bm  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
w = bench.WORKLOADS["c3"]
text, off, lens = host.synth_reference(3, w["seq_lens"], threads=16)
names = ["chr%d" % (i + 1) for i in range(len(lens))]
dev = Device(0)
dev.upload_reference([text[int(o):int(o) + int(ln)] for o, ln in zip(off, lens)])
dev.upload_reference_names(names)
dev.build_index(12, 3, fetch=False)
bases, offs = host.synth_reads(w["seed"], text, off, lens, n, w["L"], w["e"], first_read=0, threads=16)
rnames = ["SRR0000001.%d" % (i + 1) for i in range(n)]
dev.reserve_batch(n, n + n // 4, w["L"], e=w["e"])
out = {"workload": "c3", "n_reads": n, "e": w["e"]}
for level in (0, 1):
    dev.stage_reads(bases, offs)
    dev.stage_text(np.full(len(bases), ord("I"), np.uint8), rnames)
    dev.map_staged(e=w["e"])
    dev.fetch_bam(level=level)  # (warm)
    dev.stage_reads(bases, offs)
    dev.stage_text(np.full(len(bases), ord("I"), np.uint8), rnames)
    dev.map_staged(e=w["e"])
    dev.set_timing(True)
    dev.reset_timing()
    data, raw_len, n_blocks, n_rec, _, _ = dev.fetch_bam(level=level)
    out["level%d" % level] = {"kernel11_ms_per_M": dev.kernel_time(11)[0] * 1e6 / n, "kernel12_ms_per_M": dev.kernel_time(12)[0] * 1e6 / n,
                              "bytes_per_read": len(data) / n, "raw_bytes_per_read": raw_len / n, "members": n_blocks, "records": n_rec}
    dev.set_timing(False)
text_sam = dev.fetch_sam()[0]
out["sam_bytes_per_read"] = len(text_sam) / n
rng = np.random.default_rng(1)
for profile in ("illumina", "walk"):
    payload = bm.sam_to_bam_payload(bm.synthetic_sam(rng, 20000, 100, profile), [b"chr1", b"chr2"])
    z = dev.bgzf_compress(payload, 1)
    out[profile + "_bytes_per_read"] = {"raw": len(payload) / 20000, "level1": len(z) / 20000}
dev.close()
print(json.dumps(out))
