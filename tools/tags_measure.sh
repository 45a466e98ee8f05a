#!/bin/bash
# tools/tags_measure.sh [N] [OUT] [WORKLOADS]: what the tags of FEM map --rg / --nh cost, and that they cost nothing when off.  SAM
# to /dev/null on N reads (default 32 M) of each workload (default "c3 c2").  The runs alternate, three of each: BASE's default
# path, this build's default path, this build with --rg, this build with --rg --nh.  BASE=<dir> (optional): a directory holding
# another build's FEM (and its libraries): the build a change is compared against.  Each run's mapping phase is FEM's own `Time:`
# line.  Then the first million reads of each workload to a file, by default and with the switches: bytes and lines of text.
# Run from the repository root; results in OUT (default build/tags_measure).  The input files go to a fresh temporary directory,
# removed at the end.  Each GPU step has its own time limit; the first failure ends it.
set -o pipefail
N=${1:-32000000}
O=${2:-build/tags_measure}
WL=${3:-c3 c2}
RG='@RG\tID:lane1\tSM:sample1\tPL:ILLUMINA'
mkdir -p "$O"
D=$(mktemp -d) || exit 1
trap 'rm -rf "$D"' EXIT
run() {  # run NAME FEM E READS OUT ARGS...
  local name=$1 fem=$2 e=$3 reads=$4 out=$5
  shift 5
  local tm
  FEM_STAGE_TIMES=1 timeout -k 10 900 "$fem" map -e "$e" -t 16 --ref "$D/ref.fa" --index "$D/ref.idx" --read1 "$reads" -o "$out" "$@" 2> "$O/$name.err"
  local rc=$?
  [ $rc -eq 0 ] || { echo "FEM map $name failed: $rc"; tail "$O/$name.err"; exit $rc; }
  tm=$(sed -n 's/^Time: \([0-9.]*\)s$/\1/p' "$O/$name.err")
  [ -n "$tm" ] || { echo "FEM map $name: no Time: line"; exit 1; }
  echo "$name: mapping $tm s" | tee -a "$O/summary.txt"
}
for W in $WL; do
  E=$(python -c "import bench; print(bench.WORKLOADS['$W']['e'])") || exit 1
  timeout -k 10 1200 python tools/e2e_files.py "$W" "$N" "$D" > "$O/files.$W.log" 2>&1 || { echo "e2e_files failed"; tail "$O/files.$W.log"; exit 1; }
  echo "== $W: $N reads, -e $E" | tee -a "$O/summary.txt"
  for k in 1 2 3; do
    [ -n "$BASE" ] && run "$W.base.$k" "$BASE/FEM" "$E" "$D/reads.fq" /dev/null
    run "$W.off.$k" fem_amd/csrc/FEM "$E" "$D/reads.fq" /dev/null
    run "$W.rg.$k" fem_amd/csrc/FEM "$E" "$D/reads.fq" /dev/null --rg "$RG"
    run "$W.rg_nh.$k" fem_amd/csrc/FEM "$E" "$D/reads.fq" /dev/null --rg "$RG" --nh
  done
  head -n 4000000 "$D/reads.fq" > "$D/small.fq"
  run "$W.bytes.off" fem_amd/csrc/FEM "$E" "$D/small.fq" "$D/off.sam"
  run "$W.bytes.rg" fem_amd/csrc/FEM "$E" "$D/small.fq" "$D/rg.sam" --rg "$RG"
  run "$W.bytes.rg_nh" fem_amd/csrc/FEM "$E" "$D/small.fq" "$D/rg_nh.sam" --rg "$RG" --nh
  for v in off rg rg_nh; do
    echo "$W.$v: 1000000 reads, $(grep -vc '^@' "$D/$v.sam") lines, $(stat -c %s "$D/$v.sam") bytes" | tee -a "$O/summary.txt"
  done
  rm -f "$D"/*.sam "$D/small.fq" "$D/reads.fq" "$D/ref.fa" "$D/ref.idx"
done
