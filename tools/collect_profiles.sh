#!/bin/bash
# Developer tool (GPU box, from the repo root): every profile the round's documents cite, summaries only, under $PROFILE_OUT
# (default profile_out/; the profiling helpers it calls keep their own output folders).
#   bash tools/collect_profiles.sh r03 [part]     part: all (default) | bench | traffic | mfma | workloads
R=${1:-rXX}
PART=${2:-all}
O=${PROFILE_OUT:-profile_out}
cd $GRAFT_REPO_ROOT
mkdir -p $O
if [ "$PART" = all ] || [ "$PART" = bench ]; then
  python bench.py --full > $O/${R}_g_bench_journal-1pct_plain.json 2> $O/${R}_g.err
  python bench.py --gpus 1 --steps 20 --warmup 5 > $O/${R}_l_bench_journal-1pct_steps20.json 2> $O/${R}_l.err   # the driver's command
  bash tools/profile_bench.sh ${R}_b_bench_journal-1pct --full --cpu-iters 0 --no-coloring --no-fp32-operands > $O/${R}_b.log 2>&1
  bash tools/profile_bench.sh ${R}_a_coloring_journal-1pct --full --cpu-iters 0 --steps 20 --warmup 5 --no-fp32-operands --no-coloring-warm > $O/${R}_a.log 2>&1
  python tools/spmm_bench.py journal-1pct > $O/${R}_f_spmm_micro.log 2>&1
  MMW_BENCH_LANCZOS=1 python tools/spmm_bench.py journal-1pct >> $O/${R}_f_spmm_micro.log 2>&1
  MMW_STAMPS=1 MMW_BENCH_FIRST=1 MMW_BENCH_MODES=2 python tools/spmm_bench.py journal-1pct >> $O/${R}_f_spmm_micro.log 2>&1
  MMW_SD_STAMPS=1 python tools/probe_first.py full 48 2>&1 | grep -i stamps | tail -2 >> $O/${R}_f_spmm_micro.log
fi
if [ "$PART" = all ] || [ "$PART" = traffic ]; then bash tools/pmc_traffic.sh ${R}_c > $O/${R}_c.log 2>&1; fi
if [ "$PART" = all ] || [ "$PART" = mfma ]; then bash tools/pmc_mfma.sh ${R}_e > $O/${R}_e.log 2>&1; fi
if [ "$PART" = all ] || [ "$PART" = workloads ]; then
  for w in er-1pct er-50k er-5pct-2k journal-native; do
    bash tools/profile_bench.sh ${R}_d_bench_$w --full --workload $w --cpu-iters 0 --no-coloring --no-fp32-operands > $O/${R}_d_$w.log 2>&1
  done
  python bench.py --full --workload er-5pct-2k --instances-per-gpu 8 --cpu-iters 0 > $O/${R}_h_bench_er-5pct-2k_x8.json 2> $O/${R}_h.err
  python bench.py --full --gpus 2 --backend gloo --single-device --workload er-5pct-2k --instances-per-gpu 4 --cpu-iters 0 > $O/${R}_i_bench_2ranks_1gpu.json 2> $O/${R}_i.err
fi
ls -la $O | tail -30
