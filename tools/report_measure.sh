#!/bin/bash
# tools/report_measure.sh [N] [OUT] [PART]: the cost of FEM map --strata / --max-hits, and what the filter saves.  SAM to
# /dev/null on N C3 reads (default 32 M; PART sam), on the same number of reads on the repeat-rich c3r reference (PART rich) and
# on N / 2 read pairs of tools/paired_files.py with --rescue 8 (PART pairs).  The runs alternate, three of each: BASE's default
# path, this build's default path, this build with --max-hits 1, this build with --strata 0.  BASE=<dir> (optional): a
# directory holding another build's FEM (and its libraries): the build a change is compared against.  Each run's mapping
# phase is FEM's own `Time:` line, with FEM_STAGE_TIMES=1's stage lines beside it.  PART kernels: tools/report_measure.py
# (kernel times and bytes per 1 M reads).  PART defaults to all four.  Run from the repository root; results in OUT (default
# build/report_measure).  The input files go to a fresh temporary directory, removed at the end.  Each GPU step has its own
# time limit; the first failure ends it.
set -o pipefail
N=${1:-32000000}
O=${2:-build/report_measure}
PART=${3:-all}
mkdir -p "$O"
D=$(mktemp -d) || exit 1
trap 'rm -rf "$D"' EXIT
E=$(python -c "import bench; print(bench.WORKLOADS['c3']['e'])") || exit 1
run() {  # run NAME FEM REFDIR ARGS...
  local name=$1 fem=$2 ref=$3
  shift 3
  local t0 t1 rc tm
  t0=$(date +%s.%N)
  FEM_STAGE_TIMES=1 timeout -k 10 900 "$fem" map -e "$E" -t 16 --ref "$ref/ref.fa" --index "$ref/ref.idx" -o /dev/null "$@" 2> "$O/$name.err"
  rc=$?
  t1=$(date +%s.%N)
  [ $rc -eq 0 ] || { echo "FEM map $name failed: $rc"; tail "$O/$name.err"; exit $rc; }
  tm=$(sed -n 's/^Time: \([0-9.]*\)s$/\1/p' "$O/$name.err")
  [ -n "$tm" ] || { echo "FEM map $name: no Time: line"; exit 1; }
  echo "$name: $(python -c "print('mapping %.3f s, %.1f Mreads/s (process %.2f s)' % ($tm, $N / 1e6 / $tm, $t1 - $t0))")" | tee -a "$O/summary.txt"
  grep -E "stage busy|filtered lines|number of mapping" "$O/$name.err" >> "$O/summary.txt"
}
variants() {  # variants PREFIX REFDIR ARGS...: BASE's default path (if given), this build's, --max-hits 1, --strata 0
  local pre=$1 ref=$2
  shift 2
  [ -n "$BASE" ] && run "$pre.base.$k" "$BASE/FEM" "$ref" "$@"
  run "$pre.$k" fem_amd/csrc/FEM "$ref" "$@"
  run "$pre.max_hits_1.$k" fem_amd/csrc/FEM "$ref" "$@" --max-hits 1
  run "$pre.strata_0.$k" fem_amd/csrc/FEM "$ref" "$@" --strata 0
}
if [ "$PART" = all ] || [ "$PART" = sam ]; then
  timeout -k 10 1200 python tools/e2e_files.py c3 "$N" "$D" > "$O/files.log" 2>&1 || { echo "e2e_files failed"; tail "$O/files.log"; exit 1; }
  for k in 1 2 3; do variants sam "$D" --read1 "$D/reads.fq"; done
  rm -f "$D/reads.fq" "$D/ref.fa" "$D/ref.idx"
fi
if [ "$PART" = all ] || [ "$PART" = rich ]; then
  timeout -k 10 1200 python tools/report_measure.py files "$N" "$D/r" > "$O/rfiles.log" 2>&1 || { echo "c3r files failed"; tail "$O/rfiles.log"; exit 1; }
  for k in 1 2 3; do variants rich "$D/r" --read1 "$D/r/reads.fq"; done
  rm -rf "$D/r"
fi
if [ "$PART" = all ] || [ "$PART" = pairs ]; then
  P=$((N / 2))
  timeout -k 10 1200 python tools/paired_files.py "$P" "$D/p" > "$O/pfiles.log" 2>&1 || { echo "paired_files failed"; tail "$O/pfiles.log"; exit 1; }
  for k in 1 2 3; do variants pairs "$D/p" --read1 "$D/p/r1.fq" --read2 "$D/p/r2.fq" --rescue 8; done
fi
if [ "$PART" = all ] || [ "$PART" = kernels ]; then
  timeout -k 10 1100 python tools/report_measure.py 1000000 > "$O/kernels.json" 2> "$O/kernels.err" || { echo "report_measure.py failed"; tail "$O/kernels.err"; exit 1; }
  cat "$O/kernels.json"
fi
