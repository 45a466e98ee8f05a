"""tools/overlap_measure.py: the device time of the trim stage (timing id 19: the adapter match, the mates' overlap, clip points, the
scan of the kept lengths, the gather) of one batch of the 300-pair case of tests/adapter_model.py with and without
fem_dev_set_pair_overlap, alone and beside the adapter and the quality trim ("Measured").  Run from the repository's
root on a GPU; one line per setting: the entries per batch, the median, the least and the most of ten batches after two."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from oracle import fem_oracle as fo  # noqa: E402
from tests import adapter_model as am  # noqa: E402
from tests.harness import open_device  # noqa: E402

SETTINGS = (("nothing set", None, None, (0, 0, 0)), ("--trim-overlap alone", (20, 10), None, (0, 0, 0)),
            ("--adapter alone", None, am.A1, (0, 0, 0)), ("--adapter and --trim-overlap", (20, 10), am.A1, (0, 0, 0)),
            ("--trim-qual 20 alone", None, None, (0, 0, 20)), ("--trim-qual 20 and --trim-overlap", (20, 10), None, (0, 0, 20)))


def main():
    p = am.pairs_case()
    dev = open_device(p["seqs"], p["names"], p["idx"])[0]
    dev.set_pairs(0, 500)
    dev.set_timing(True)
    batch = fo.ReadBatch(p["reads"])
    q = np.frombuffer("".join(p["quals"]).encode("latin-1"), np.uint8)
    names2 = p["rnames"] + p["rnames"]
    for tag, overlap, adapter, trim in SETTINGS:
        dev.set_trim(*trim)
        dev.set_adapter(adapter, am.A2 if adapter else None)
        if overlap:
            dev.set_pair_overlap(*overlap)
        else:
            dev.set_pair_overlap(None)
        times = []
        for rep in range(12):
            dev.reset_timing()
            dev.stage_reads(batch.bases, batch.off)
            dev.stage_text(q, names2)
            dev.map_staged(e=p["e"])
            dev.fetch()
            if rep >= 2:
                times.append(dev.kernel_time(19))
        ms = [t[0] for t in times]
        print("%-36s stage 19: entries per batch %d, median %.1f us, min %.1f us, max %.1f us"
              % (tag, times[0][1], 1e3 * statistics.median(ms), 1e3 * min(ms), 1e3 * max(ms)), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
