#!/bin/bash
# Round measurements on an MI355X:  bash tools/measure_round.sh r02a [OUTDIR]   -> OUTDIR/<tag>_*, OUTDIR defaults to measure_out/
# (copy the summaries into profiles/)
set -x
TAG=${1:-r02}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd $ROOT
OUT=$(mkdir -p "${2:-measure_out}" && cd "${2:-measure_out}" && pwd)
export D4_GEMM_TUNE_CACHE=$OUT/tune_cache_$TAG.txt
rm -f $D4_GEMM_TUNE_CACHE
# 1. the full bench (headline + roofline + baselines + secondary keys), then the driver-style torchrun launch with the 1-rank RCCL group forced
timeout 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
D4_FORCE_PG=1 NCCL_DEBUG=INFO python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus 1 --steps 3 --warmup 2 --full --no-cpu-baseline --no-secondary > $OUT/${TAG}_bench_rccl1.json 2> $OUT/${TAG}_bench_rccl1.err
cat $OUT/${TAG}_bench_rccl1.err $OUT/${TAG}_bench_rccl1.json | grep -i "NCCL INFO" | grep -i "init\|comm\|version\|Using\|Channel" | head -30 > $OUT/${TAG}_rccl_init.log
# 2. kernel trace + stats of the same command
cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o bench -- python $ROOT/bench.py --gpus 1 --steps 5 --warmup 2 --full --no-cpu-baseline --no-secondary > $OUT/${TAG}_bench_profiled.json 2> /dev/null
rm -f $OUT/${TAG}_prof/bench_kernel_trace.csv
# 3. PMC passes over a short rollout (no tuning launches: cache present)
for pass in "FETCH_SIZE GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES" "WRITE_SIZE SQ_WAIT_INST_ANY SQ_LDS_BANK_CONFLICT SQ_WAIT_ANY"; do
  tag=$(echo $pass | cut -d' ' -f1)
  timeout 400 rocprofv3 --kernel-trace --pmc $pass --output-format csv -d $OUT/pmc_$tag -o p -- python $ROOT/tools/rollout_profile_target.py > /dev/null 2>&1
done
cd $ROOT
python tools/pmc_summary.py $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE --json $OUT/${TAG}_pmc_traffic.json > $OUT/${TAG}_rollout_pmc.txt
rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE
cp $D4_GEMM_TUNE_CACHE $OUT/${TAG}_gemm_tile_choices.txt
head -8 $OUT/${TAG}_rollout_pmc.txt | cut -c1-220
cut -c1-700 $OUT/${TAG}_bench.json
tail -3 $OUT/${TAG}_bench_rccl1.err; cut -c1-300 $OUT/${TAG}_bench_rccl1.json; head -5 $OUT/${TAG}_rccl_init.log
