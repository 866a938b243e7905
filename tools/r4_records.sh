#!/bin/bash
# r4_records.sh -- the round-4 records kept under profiles/: PMC + kernel stats of the headline bench, the
# default bench line (with the CPU baseline), variant 4b, config 4 / 5 as embed(), configs 2 and 3
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
O=$R/gpurun_out/r4rec; rm -rf $O; mkdir -p $O
cd $R
bash tools/pmc_traffic.sh > $O/pmc_run.log 2>&1
cp gpurun_out/pmc/pmc_traffic.json gpurun_out/pmc/kernel_stats.csv $O/ 2>/dev/null
cp $R/gpurun_out/pmc/pmc_traffic.json $R/profiles/r04_pmc_traffic.json 2>/dev/null   # (the bench lines below pick it up)
python bench.py --full 2>/dev/null | tail -1 > $O/bench_line.json
python bench.py --full --no-cpu-baseline --variant 4b 2>/dev/null | tail -1 > $O/config4b_bench_line.json
python bench.py --config 4 --embed 2>/dev/null | tail -1 > $O/config4_embed_bench_line.json
bash tools/prof_cmd.sh c4embed python $R/bench.py --config 4 --embed > $O/config4_embed_kernels.txt 2>&1
cp gpurun_out/c4embed_kernel_stats.csv $O/config4_embed_kernel_stats.csv 2>/dev/null
python bench.py --config 2 2>/dev/null | tail -1 > $O/config2_bench_line.json
python bench.py --config 3 2>/dev/null | tail -1 > $O/config3_bench_line.json
python bench.py --config 5 2>/dev/null | tail -1 > $O/config5_bench_line.json
python bench.py --config 5 --embed 2>/dev/null | tail -1 > $O/config5_embed_bench_line.json
for W in 2 4 8; do python bench.py --full --no-cpu-baseline --emulate-world $W --steps 50 --blocks 5 2>/dev/null | tail -1 > $O/shard_W$W.json; done
ls -la $O
