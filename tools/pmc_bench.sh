#!/bin/bash
# Runs on the MI355X from the repo root: kernel stats + HBM traffic counters of the bench command, then the bench itself with the
# sidecar so that roofline.traffic is measured by THIS session. Counters are collected in their own passes (--kernel-trace only, never with other
# trace domains). usage: [OUT=dir] tools/pmc_bench.sh [round tag, default r05]
# Outputs under $OUT (default prof_out/): <tag>_kernel_stats.csv, <tag>_pmc_sidecar.json, <tag>_pmc_raw.csv, <tag>_bench_request.log, <tag>_bench_sketch.log
T=${1:-r05}
R=$(pwd)
mkdir -p "${OUT:-prof_out}"; O=$(cd "${OUT:-prof_out}" && pwd)
export TMPDIR=/tmp
export GS_HEAD=$(cat $R/.head 2>/dev/null)
RX='k_hnsw_search|k_match_join|k_sketch_min|k_hamming_qxc'
# --full: the gather-mode roofline search (k_hnsw_search) is one of the launches the sidecar prices
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_stats -o $T -- python $R/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --no-extra-legs > $O/${T}_bench_under_rocprof.log 2>&1
rocprofv3 --kernel-trace --output-format csv --pmc FETCH_SIZE --kernel-include-regex "$RX" -d $O/pmc_fetch -- python $R/bench.py --steps 1 --warmup 1 --full --no-cpu-baseline --no-extra-legs > /dev/null 2>&1
rocprofv3 --kernel-trace --output-format csv --pmc WRITE_SIZE --kernel-include-regex "$RX" -d $O/pmc_write -- python $R/bench.py --steps 1 --warmup 1 --full --no-cpu-baseline --no-extra-legs > /dev/null 2>&1
# configs[4] distance leg (u64 row gather): the same launch the bench's extra leg times
rocprofv3 --kernel-trace --output-format csv --pmc FETCH_SIZE --kernel-include-regex 'k_hnsw_search<2>' -d $O/pmc_c5f -- python $R/bench.py --workload c5dist > /dev/null 2>&1
rocprofv3 --kernel-trace --output-format csv --pmc WRITE_SIZE --kernel-include-regex 'k_hnsw_search<2>' -d $O/pmc_c5w -- python $R/bench.py --workload c5dist > /dev/null 2>&1
cd $R
python tools/pmc_condense.py $O/pmc_fetch $O/pmc_write $O/${T}_pmc_sidecar.json $O/${T}_pmc_raw.csv $O/pmc_c5f $O/pmc_c5w > $O/${T}_pmc_condense.log 2>&1
S=$(find $O/prof_stats -name "*kernel_stats.csv" | head -1); [ -n "$S" ] && cp "$S" $O/${T}_kernel_stats.csv
rm -rf $O/prof_stats $O/pmc_fetch $O/pmc_write $O/pmc_c5f $O/pmc_c5w
GS_PMC_SIDECAR=$O/${T}_pmc_sidecar.json python bench.py --steps 5 --warmup 2 --full > $O/${T}_bench_request.log 2> $O/${T}_bench_request.err
python bench.py --workload sketch --steps 3 --warmup 1 --full > $O/${T}_bench_sketch.log 2>> $O/${T}_bench_request.err
tail -c 400 $O/${T}_pmc_condense.log; head -12 $O/${T}_kernel_stats.csv | cut -c1-160
