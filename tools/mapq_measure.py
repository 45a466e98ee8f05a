"""tools/mapq_measure.py [n_reads]: the cost of --mapq on C3 — the device time of the MAPQ kernel (id 13) and of the SAM text
kernels (id 7) per 1 M reads single-end (C3's reads), and of the pairing kernel (id 9), id 13 and id 7 per 1 M reads of read pairs
(n_reads / 2 pairs of tools/paired_files.py: fragments of 200-500 bp, so that most pairs have concordant combinations), with MAPQ
off and on.  One JSON line on stdout."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from fem_amd import Device, host  # noqa: E402
sys.path.insert(0, os.path.join(os.getcwd(), "tools"))
import paired_files  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
w = bench.WORKLOADS["c3"]
text, off, lens = host.synth_reference(3, w["seq_lens"], threads=16)
dev = Device(0)
dev.upload_reference([text[int(o):int(o) + int(ln)] for o, ln in zip(off, lens)])
dev.upload_reference_names(["chr%d" % (i + 1) for i in range(len(lens))])
dev.build_index(12, 3, fetch=False)
se_bases, se_offs = host.synth_reads(w["seed"], text, off, lens, n, w["L"], w["e"], first_read=0, threads=16)
m1, m2 = paired_files.mates(text, off, lens, n // 2)
pe_bases = np.concatenate([m1.reshape(-1), m2.reshape(-1), np.zeros(8, np.uint8)])
pe_offs = (np.arange(2 * (n // 2) + 1, dtype=np.uint64) * np.uint64(paired_files.L))
rnames = ["SRR0000001.%d" % (i + 1) for i in range(n)]
dev.reserve_batch(n, n + n // 4, w["L"], e=w["e"])
out = {"workload": "c3", "n_reads": n, "e": w["e"], "pairs": n // 2}


def timed(kernels, bases, offs):
    quals = np.full(len(bases), ord("I"), np.uint8)
    names = rnames[:len(offs) - 1]
    dev.stage_reads(bases, offs)
    dev.stage_text(quals, names)
    dev.map_staged(e=w["e"])
    dev.fetch_sam()  # (warm)
    dev.stage_reads(bases, offs)
    dev.stage_text(quals, names)
    dev.map_staged(e=w["e"])
    dev.set_timing(True)
    dev.reset_timing()
    dev.fetch_sam()
    r = {"kernel%d_ms_per_M" % k: dev.kernel_time(k)[0] * 1e6 / n for k in kernels}
    r["text_ms_per_M"] = dev.kernel_time(7)[0] * 1e6 / n
    dev.set_timing(False)
    return r


for pairs in (False, True):
    dev.set_pairs(0, 500) if pairs else dev.set_pairs(None)
    for on in (False, True):
        dev.set_mapq(on)
        r = timed((9, 13) if pairs else (13,), pe_bases if pairs else se_bases, pe_offs if pairs else se_offs)
        if pairs:
            r["proper_pairs"] = dev.pair_count()
        out["%s_mapq_%s" % ("pairs" if pairs else "single", "on" if on else "off")] = r
dev.close()
print(json.dumps(out))
