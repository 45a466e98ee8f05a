"""tools/coverage_measure.py: the device time of the coverage stage (coverage_kernel, fem_dbg_stage_ms stage 12) beside that of the
same fetch's text kernels (stage 3), for one batch of a repeat case (every read on the same 130 loci: the adds of a batch meet in
a few bins) and one of a random case, at W = 1000 and W = 1, primary lines and all hits ("Measured").  Run from
the repository's root on a GPU; one line per setting: the lines of the text, and the median, the least and the most of ten
batches after two, for both stages."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
from fem_amd.device import STAGE_COVERAGE, STAGE_TEXT  # noqa: E402
from tests import cases, util  # noqa: E402
from tests.harness import open_device, stage_and_map  # noqa: E402

L, E = 100, 3


def repeat_case(rng, n):
    seqs, names, units, _, _ = cases.report_reference(rng, L, copies=(130, 2))
    seqs, names = seqs[2:4], names[2:4]
    u130 = units[0][0]
    return seqs, names, [u130[o:o + L] for o in rng.integers(0, 61, n)]


def random_case(rng, n):
    seqs, names = cases.reference(rng, False)
    return seqs, names, util.make_reads(rng, seqs, n, L, E)


def main():
    rng = np.random.default_rng(815)
    for tag, maker, n in (("repeat", repeat_case, 2000), ("random", random_case, 100_000)):
        seqs, names, reads = maker(rng, n)
        rnames, quals = ["r%d" % i for i in range(len(reads))], cases.quals(reads)
        dev = open_device(seqs, names)[0]
        for W in (1000, 1):
            for all_hits in (False, True):
                dev.set_coverage(W, all_hits)
                cov, text, lines = [], [], 0
                for rep in range(12):
                    stage_and_map(dev, reads, rnames, quals, E)
                    lines = dev.fetch_sam()[0].count(b"\n")
                    if rep >= 2:
                        cov.append(1e3 * dev.stage_ms(STAGE_COVERAGE))
                        text.append(1e3 * dev.stage_ms(STAGE_TEXT))
                covered = int(dev.fetch_coverage().sum())
                print("%-6s W %-4d %-8s %7d reads %8d lines %11d bases/batch  coverage: median %.1f us (%.1f-%.1f)  text: median %.1f us (%.1f-%.1f)"
                      % (tag, W, "all" if all_hits else "primary", len(reads), lines, covered // 12, statistics.median(cov), min(cov), max(cov),
                         statistics.median(text), min(text), max(text)), flush=True)
        dev.close()


if __name__ == "__main__":
    main()
