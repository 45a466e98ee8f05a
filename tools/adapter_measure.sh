#!/bin/bash
# tools/adapter_measure.sh [N] [OUT] [PART]: what FEM map --adapter costs when off, and what it costs when on.  SAM to /dev/null at
# -t 16, N C3 reads (default 16 M), three runs each, by turns.  PART off: BASE's FEM and this build's without the switches
# (BASE=<dir>: a directory holding another build's FEM and its libraries, the build a change is compared against; without it this
# build alone).  PART adapter: this build with --trim-qual 20 alone and with --trim-qual 20 --adapter (the generator plants no
# adapter, so the match leaves no read early: its worst case).  PART kernels: tools/adapter_measure.py (the trim stage's device time
# per million reads with the adapter match in it, beside the fixed trims alone and the mapping's kernels).  PART defaults to all
# three.  Run from the repository root; results in OUT (default build/adapter_measure).  The input files go to a fresh temporary
# directory, removed at the end.  Each GPU step has its own time limit; the first failure ends it.
set -o pipefail
N=${1:-16000000}
O=${2:-build/adapter_measure}
A=AGATCGGAAGAGCACACGTCTGAACTCCAGTCA
PART=${3:-all}
mkdir -p "$O"
D=$(mktemp -d) || exit 1
trap 'rm -rf "$D"' EXIT
E=$(python -c "import bench; print(bench.WORKLOADS['c3']['e'])") || exit 1
run() {  # run NAME FEM ARGS...
  local name=$1 fem=$2
  shift 2
  local rc tm
  timeout -k 10 600 "$fem" map -e "$E" -t 16 --ref "$D/ref.fa" --index "$D/ref.idx" --read1 "$D/reads.fq" -o /dev/null "$@" 2> "$O/$name.err"
  rc=$?
  [ $rc -eq 0 ] || { echo "FEM map $name failed: $rc"; tail "$O/$name.err"; exit $rc; }
  tm=$(sed -n 's/^Time: \([0-9.]*\)s$/\1/p' "$O/$name.err")
  [ -n "$tm" ] || { echo "FEM map $name: no Time: line"; exit 1; }
  echo "$name: $(python -c "print('mapping %.3f s, %.1f Mreads/s' % ($tm, $N / 1e6 / $tm))")" | tee -a "$O/summary.txt"
  grep -E "trimmed|adapter|number of mapping" "$O/$name.err" >> "$O/summary.txt"
}
if [ "$PART" != kernels ]; then
  timeout -k 10 1000 python tools/e2e_files.py c3 "$N" "$D" > "$O/files.log" 2>&1 || { echo "e2e_files failed"; tail "$O/files.log"; exit 1; }
fi
if [ "$PART" = all ] || [ "$PART" = off ]; then
  for k in 1 2 3; do
    [ -n "$BASE" ] && run "off.base.$k" "$BASE/FEM"
    run "off.this.$k" fem_amd/csrc/FEM
  done
fi
if [ "$PART" = all ] || [ "$PART" = adapter ]; then
  for k in 1 2 3; do
    run "adapter.qual.$k" fem_amd/csrc/FEM --trim-qual 20
    run "adapter.both.$k" fem_amd/csrc/FEM --trim-qual 20 --adapter "$A"
  done
fi
rm -f "$D/reads.fq" "$D/ref.fa" "$D/ref.idx"
if [ "$PART" = all ] || [ "$PART" = kernels ]; then
  timeout -k 10 600 python tools/adapter_measure.py 1000000 > "$O/kernels.json" 2> "$O/kernels.err" || { echo "adapter_measure.py failed"; tail "$O/kernels.err"; exit 1; }
  cat "$O/kernels.json"
fi
