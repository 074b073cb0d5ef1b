set -e
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-/tmp/spfm_out}  # where the results go
mkdir -p "$OUT"
cd $R
timeout -k 10 500 python bench.py --full --steps 5 --warmup 1 > $OUT/v6_bench.json 2> $OUT/v6_bench.err
tail -c 1500 $OUT/v6_bench.json
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_v6 -o run -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > $OUT/v6_bench_under_rocprof.json 2> $OUT/v6_rocprof.err
cp /tmp/prof_v6/run_kernel_stats.csv $OUT/v6_kernel_stats.csv
head -6 $OUT/v6_kernel_stats.csv | cut -c1-200
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d /tmp/pmc_f -o run -- python $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > /dev/null 2> $OUT/v6_pmc_f.err
python $R/tools/pmc_summary.py /tmp/pmc_f > $OUT/v6_pmc_fetch_summary.txt
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d /tmp/pmc_w -o run -- python $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > /dev/null 2> $OUT/v6_pmc_w.err
python $R/tools/pmc_summary.py /tmp/pmc_w > $OUT/v6_pmc_write_summary.txt
head -5 $OUT/v6_pmc_fetch_summary.txt $OUT/v6_pmc_write_summary.txt
