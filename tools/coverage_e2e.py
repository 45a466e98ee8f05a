"""tools/coverage_e2e.py <c2|c3> <n_reads> [rounds]: FEM map to /dev/null on generated files (those of tools/e2e_probe.py) without
and with --coverage (W = 1000, the file into the same temporary directory), by turns, each run's `Time:` (the mapping phase, the
fetch and the writing of the track included) and the covered bases ("Measured")."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from fem_amd import host  # noqa: E402


def main():
    key, n_reads = sys.argv[1], int(sys.argv[2])
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    w = bench.WORKLOADS[key]
    text, off, lens = host.synth_reference(w["seed"] if key == "c2" else 3, w["seq_lens"], threads=16)
    d = tempfile.mkdtemp(prefix="fem_cov_", dir="/dev/shm")
    exe = os.path.join(os.getcwd(), "fem_amd", "csrc", "FEM")
    try:
        fa, fq, ix, cov = (os.path.join(d, n) for n in ("ref.fa", "reads.fq", "ref.idx", "cov.bed"))
        host.write_fasta(fa, text, off, lens)
        bases, _ = host.synth_reads(w["seed"], text, off, lens, n_reads, w["L"], w["e"], first_read=0, threads=16)
        host.write_fastq(fq, bases, w["L"], n_reads)
        r = subprocess.run([exe, "index", "12", "3", fa, ix], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-300:]
        common = [exe, "map", "-e", str(w["e"]), "-t", "16", "--ref", fa, "--index", ix, "--read1", fq, "-o", "/dev/null"]
        for rnd in range(rounds):
            for tag, extra in (("plain", []), ("--coverage", ["--coverage", cov])):
                r = subprocess.run(common + extra, capture_output=True, text=True, timeout=900)
                t = re.search(r"Time: ([0-9.]+)s", r.stderr)
                c = re.search(r"covered bases: (\d+)", r.stderr)
                print("%s %d reads, round %d, %-10s rc %d Time %s s -> %.1f Mreads/s%s" % (
                    key, n_reads, rnd, tag, r.returncode, t.group(1) if t else None, n_reads / float(t.group(1)) / 1e6 if t else 0.0,
                    ", covered bases %s, %d lines of BED" % (c.group(1), sum(1 for _ in open(cov))) if c else ""), flush=True)
                if r.returncode != 0:  # nothing more is started on the card behind a run that did not end as it should
                    sys.exit("FEM map ended with %d:\n%s" % (r.returncode, r.stderr[-600:]))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
