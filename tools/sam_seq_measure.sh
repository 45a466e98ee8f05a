#!/bin/bash
# tools/sam_seq_measure.sh [OUT] [N_E2E]: what FEM map --sam-seq costs, and that it costs nothing when off.
# 1. The text stage's device time (tools/sam_seq_measure.py: SAM text kernels id 7, BAM record kernels id 11) on one batch of
#    250 000 C2 reads, five rounds, each round BASE's library then this build's (option off, then on), a process each, a warm-up
#    fetch in front of every measured one.  BASE=<dir> (optional): a directory holding another build's libfemhip.so, libfemhost.so
#    and FEM: the build a change is compared against.
# 2. FEM map end to end on N_E2E C2 reads (default 32 M) to /dev/null at -t 16 and -t 24, without and with the switch: FEM's own
#    `Time:` line (the mapping phase).  At -t 24 the qualities stay on the host without the switch and go to the device with it.
# Run from the repository root; results in OUT (default build/sam_seq_measure).  The input files go to a fresh temporary
# directory, removed at the end.  Each GPU step has its own time limit; the first failure ends it.
set -o pipefail
O=${1:-build/sam_seq_measure}
N=${2:-32000000}
mkdir -p "$O"
: > "$O/kernels.jsonl"
for k in 1 2 3 4 5; do
  if [ -n "$BASE" ]; then
    FEM_HIP_LIBRARY="$BASE/libfemhip.so" timeout -k 10 300 python tools/sam_seq_measure.py 250000 1 >> "$O/kernels.jsonl" 2> "$O/base.$k.err" || { echo "base run $k failed: $?"; tail "$O/base.$k.err"; exit 1; }
  fi
  timeout -k 10 300 python tools/sam_seq_measure.py 250000 1 >> "$O/kernels.jsonl" 2> "$O/this.$k.err" || { echo "run $k failed: $?"; tail "$O/this.$k.err"; exit 1; }
done
python - "$O/kernels.jsonl" <<'EOF' | tee "$O/summary.txt"
import json, statistics, sys
rows = [json.loads(l) for l in open(sys.argv[1]) if l.startswith("{")]
def show(name, xs):
    if xs:
        print("%-14s median %.4f ms, min %.4f, max %.4f, spread %.4f  %s" % (name, statistics.median(xs), min(xs), max(xs), max(xs) - min(xs), xs))
for key, what in (("sam_ms", "SAM id 7"), ("bam_ms", "BAM id 11")):
    print("==", what, "250000 C2 reads")
    show("base", [x for r in rows if r["library"] != "this build" for x in r["off"][key]])
    show("this, off", [x for r in rows if r["library"] == "this build" for x in r["off"][key]])
    show("this, on", [x for r in rows if r["library"] == "this build" and "on" in r for x in r["on"][key]])
last = [r for r in rows if "turned" in r]
if last:
    print("lines %d, turned %d, text bytes %d" % (last[-1]["lines"], last[-1]["turned"], last[-1]["on"]["text_bytes"]))
EOF
D=$(mktemp -d) || exit 1
trap 'rm -rf "$D"' EXIT
timeout -k 10 900 python tools/e2e_files.py c2 "$N" "$D" > "$O/files.log" 2>&1 || { echo "e2e_files failed"; tail "$O/files.log"; exit 1; }
run() {  # run NAME THREADS ARGS...
  local name=$1 t=$2
  shift 2
  timeout -k 10 600 fem_amd/csrc/FEM map -e 3 -t "$t" --ref "$D/ref.fa" --index "$D/ref.idx" --read1 "$D/reads.fq" -o /dev/null "$@" 2> "$O/$name.err"
  local rc=$?
  [ $rc -eq 0 ] || { echo "FEM map $name failed: $rc"; tail "$O/$name.err"; exit $rc; }
  echo "$name: mapping $(sed -n 's/^Time: \([0-9.]*\)s$/\1/p' "$O/$name.err") s" | tee -a "$O/summary.txt"
}
echo "== FEM map, $N C2 reads to /dev/null" | tee -a "$O/summary.txt"
for k in 1 2; do
  run "t16.off.$k" 16
  run "t16.on.$k" 16 --sam-seq
  run "t24.off.$k" 24
  run "t24.on.$k" 24 --sam-seq
done
