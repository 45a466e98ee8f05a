#!/bin/bash
# tools/bam_measure.sh [N] [OUT]: FEM map on N C3 reads (default 32 M) as SAM, --bam=0 and --bam, each to a file and to
# /dev/null, then tools/bam_measure.py.  Run from the repository root; results in OUT (default build/bam_measure).  The input
# files go to a fresh temporary directory, removed at the end.  Each GPU step has its own time limit; the first failure ends it.
set -o pipefail
N=${1:-32000000}
O=${2:-build/bam_measure}
mkdir -p "$O"
D=$(mktemp -d) || exit 1
trap 'rm -rf "$D"' EXIT
E=$(python -c "import bench; print(bench.WORKLOADS['c3']['e'])") || exit 1
timeout -k 10 1200 python tools/e2e_files.py c3 "$N" "$D" > "$O/files.log" 2>&1 || { echo "e2e_files failed"; tail "$O/files.log"; exit 1; }
for fmt in sam bam0 bam1; do
  case $fmt in sam) flag="" ;; bam0) flag="--bam=0" ;; bam1) flag="--bam" ;; esac
  for dst in file null; do
    out=/dev/null
    [ $dst = file ] && out="$D/out.$fmt"
    t0=$(date +%s.%N)
    FEM_STAGE_TIMES=1 timeout -k 10 900 fem_amd/csrc/FEM map -e "$E" -t 16 --ref "$D/ref.fa" --index "$D/ref.idx" --read1 "$D/reads.fq" \
      -o "$out" $flag 2> "$O/$fmt.$dst.err"
    rc=$?
    t1=$(date +%s.%N)
    [ $rc -eq 0 ] || { echo "FEM map $fmt $dst failed: $rc"; tail "$O/$fmt.$dst.err"; exit $rc; }
    size=0
    [ $dst = file ] && size=$(stat -c %s "$out")
    echo "$fmt $dst: $(python -c "print('%.1f s, %.1f Mreads/s, %d bytes' % ($t1 - $t0, $N / 1e6 / ($t1 - $t0), $size))")" | tee -a "$O/summary.txt"
    grep -E "stage busy|timeline|^Time:|Time:" "$O/$fmt.$dst.err" | tee -a "$O/summary.txt"
    [ $dst = file ] && rm -f "$out"
  done
done
timeout -k 10 900 python tools/bam_measure.py 1000000 > "$O/kernels.json" 2> "$O/kernels.err" || { echo "bam_measure.py failed"; tail "$O/kernels.err"; exit 1; }
cat "$O/kernels.json"
