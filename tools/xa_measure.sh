#!/bin/bash
# tools/xa_measure.sh [N] [OUT] [PART]: what FEM map --xa costs when off, and what it buys when on.  SAM to /dev/null at -t 16.
# PART off: N C3 reads (default 32 M), three runs each of BASE's FEM and this build's without the switch, by turns.  BASE=<dir>: a
# directory holding another build's FEM and its libraries, the build a change is compared against (without it this build alone).
# PART rich: N reads on the repeat-rich c3r reference, PART pairs: N / 2 read pairs of tools/paired_files.py with --rescue 8; each
# three runs without and with --xa, by turns.  Each run's mapping phase is FEM's own `Time:` line.  PART kernels: tools/xa_measure.py
# (kernel times and bytes of text per read on 1 M reads of each input).  PART defaults to all four.  Run from
# the repository root; results in OUT (default build/xa_measure).  The input files go to a fresh temporary directory, removed at
# the end.  Each GPU step has its own time limit; the first failure ends it.
set -o pipefail
N=${1:-32000000}
O=${2:-build/xa_measure}
PART=${3:-all}
mkdir -p "$O"
D=$(mktemp -d) || exit 1
trap 'rm -rf "$D"' EXIT
E=$(python -c "import bench; print(bench.WORKLOADS['c3']['e'])") || exit 1
run() {  # run NAME READS FEM REFDIR ARGS...
  local name=$1 reads=$2 fem=$3 ref=$4
  shift 4
  local rc tm
  timeout -k 10 900 "$fem" map -e "$E" -t 16 --ref "$ref/ref.fa" --index "$ref/ref.idx" -o /dev/null "$@" 2> "$O/$name.err"
  rc=$?
  [ $rc -eq 0 ] || { echo "FEM map $name failed: $rc"; tail "$O/$name.err"; exit $rc; }
  tm=$(sed -n 's/^Time: \([0-9.]*\)s$/\1/p' "$O/$name.err")
  [ -n "$tm" ] || { echo "FEM map $name: no Time: line"; exit 1; }
  echo "$name: $(python -c "print('mapping %.3f s, %.1f Mreads/s' % ($tm, $reads / 1e6 / $tm))")" | tee -a "$O/summary.txt"
  grep -E "XA entries|number of mapping" "$O/$name.err" >> "$O/summary.txt"
}
with_and_without() {  # with_and_without PREFIX READS REFDIR ARGS...
  local pre=$1 reads=$2 ref=$3
  shift 3
  for k in 1 2 3; do
    run "$pre.plain.$k" "$reads" fem_amd/csrc/FEM "$ref" "$@"
    run "$pre.xa.$k" "$reads" fem_amd/csrc/FEM "$ref" "$@" --xa
  done
}
if [ "$PART" = all ] || [ "$PART" = off ]; then
  timeout -k 10 1200 python tools/e2e_files.py c3 "$N" "$D" > "$O/files.log" 2>&1 || { echo "e2e_files failed"; tail "$O/files.log"; exit 1; }
  for k in 1 2 3; do
    [ -n "$BASE" ] && run "off.base.$k" "$N" "$BASE/FEM" "$D" --read1 "$D/reads.fq"
    run "off.this.$k" "$N" fem_amd/csrc/FEM "$D" --read1 "$D/reads.fq"
  done
  rm -f "$D/reads.fq" "$D/ref.fa" "$D/ref.idx"
fi
if [ "$PART" = all ] || [ "$PART" = rich ]; then
  timeout -k 10 1200 python tools/report_measure.py files "$N" "$D/r" > "$O/rfiles.log" 2>&1 || { echo "c3r files failed"; tail "$O/rfiles.log"; exit 1; }
  with_and_without rich "$N" "$D/r" --read1 "$D/r/reads.fq"
  rm -rf "$D/r"
fi
if [ "$PART" = all ] || [ "$PART" = pairs ]; then
  P=$((N / 2))
  timeout -k 10 1200 python tools/paired_files.py "$P" "$D/p" > "$O/pfiles.log" 2>&1 || { echo "paired_files failed"; tail "$O/pfiles.log"; exit 1; }
  with_and_without pairs "$N" "$D/p" --read1 "$D/p/r1.fq" --read2 "$D/p/r2.fq" --rescue 8
fi
if [ "$PART" = all ] || [ "$PART" = kernels ]; then
  timeout -k 10 1100 python tools/xa_measure.py 1000000 > "$O/kernels.json" 2> "$O/kernels.err" || { echo "xa_measure.py failed"; tail "$O/kernels.err"; exit 1; }
  cat "$O/kernels.json"
fi
