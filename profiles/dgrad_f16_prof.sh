set -uo pipefail
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${DCUE_PROF_OUT:-$ROOT/profiles/out}/dgrad_f16
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
for V in 0 1; do
  DCUE_DGRAD_F16=$V timeout -k 10 200 rocprofv3 --kernel-trace --stats -f csv -d "$OUT/trace_$V" -o run -- python3 $ROOT/bench.py --full --no-cpu-baseline --no-eval --steps 50 --warmup 10 --modes catalogue --profile-phase catalogue > "$OUT/dgprof_$V.log" 2>&1 || exit 1
  f=$(find "$OUT/trace_$V" -name '*kernel_stats.csv' | head -n 1)
  grep -E 'k_conv_rows<1' "$f" | cut -c1-160 > "$OUT/dgprof_$V.txt"
done
cat "$OUT/dgprof_0.txt" "$OUT/dgprof_1.txt"
