#!/bin/bash
# end-of-round check: the whole GPU suite, smoke, the full default bench (profiles/r06_bench_default.log), the 5-step request bench (profiles/r06_bench_request.log)
# outputs under $OUT (default prof_out/)
cd "$(dirname "$0")/.."
O=${OUT:-prof_out}; mkdir -p $O
timeout 3000 python -m pytest tests -m gpu -q -x 2>&1 | grep -E "passed|failed|error" | tail -3 > $O/final_suite.txt
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -1 >> $O/final_suite.txt
timeout 1500 python -u bench.py --full > $O/final_bench_default.log 2> $O/final_bench_default.err
timeout 900 python -u bench.py --steps 5 --warmup 2 --full --no-extra-legs > $O/final_bench_request.log 2> $O/final_bench_request.err
cat $O/final_suite.txt
python tools/skew_summary.py $O/final_bench_default.log
python tools/bench_summary.py default < $O/final_bench_default.log
python tools/bench_summary.py request < $O/final_bench_request.log
