# rocprofv3 kernel stats of the headline bench + the full bench line (roofline, whole-MEX and host-call legs, CPU
# baselines), on a machine with an MI355X.  Results land in $OUT (default prof_out/ in the repository root).
set -e
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT="${OUT:-prof_out}"
mkdir -p "$OUT"
python3 bench.py --full > "$OUT"/bench_default.json 2> "$OUT"/bench_default.err
grep "^{" "$OUT"/bench_default.json | cut -c1-250
rm -rf "$OUT"/prof_epi
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_epi -- python3 bench.py --full --no-cpu-baseline > "$OUT"/prof_epi.log 2>&1
S=$(find "$OUT"/prof_epi -name "*kernel_stats.csv" | head -1)
cp $S "$OUT"/prof_epi_kernel_stats.csv
cut -c1-160 "$OUT"/prof_epi_kernel_stats.csv | head -8
grep "^{" "$OUT"/prof_epi.log | cut -c1-200
rm -rf "$OUT"/prof_epi
