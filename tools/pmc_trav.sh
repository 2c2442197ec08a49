#!/bin/bash
# Runs ON the GPU box, from the repository root: SQ counters of k_hnsw_search_dense over one bench-sized request (tools/trav_ab.py --genomes: 300 k genomes,
# 10 000 queries, ef 5000), counters only, two passes of eight; condensed by tools/pmc_kernel.py together with the pops per query that trav_ab prints, so that
# wave-instructions per pop can be read off one file. Each pass runs under its own time limit and a pass that fails ends the script.
# usage: tools/pmc_trav.sh <tag> [output directory, default profiles/]   -> <output directory>/<tag>_trav_pmc.txt
set -o pipefail
T=${1:-trav}; R=$(pwd); O=$(mkdir -p "${2:-profiles}" && cd "${2:-profiles}" && pwd) || exit 1; export TMPDIR=/tmp
RX="k_hnsw_search_dense"
cd /tmp
timeout -k 10 420 rocprofv3 --kernel-trace --output-format csv --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_WAVE_CYCLES --kernel-include-regex "$RX" -d $O/pmc_t1 -- python $R/tools/trav_ab.py --genomes --reps 1 "" > $O/pmc_t1.log 2>&1 || { tail -20 $O/pmc_t1.log; exit 1; }
timeout -k 10 420 rocprofv3 --kernel-trace --output-format csv --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INST_CYCLES_SALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_BUSY_CYCLES --kernel-include-regex "$RX" -d $O/pmc_t2 -- python $R/tools/trav_ab.py --genomes --reps 1 "" > $O/pmc_t2.log 2>&1 || { tail -20 $O/pmc_t2.log; exit 1; }
cd $R
{ python tools/pmc_kernel.py "$RX" $O/pmc_t1 $O/pmc_t2; grep -h "traversal\|evals/query" $O/pmc_t1.log; } > $O/${T}_trav_pmc.txt 2>&1
rm -rf $O/pmc_t1 $O/pmc_t2 $O/pmc_t1.log $O/pmc_t2.log; cat $O/${T}_trav_pmc.txt
