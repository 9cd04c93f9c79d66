set -x
# usage: tools/final_measure_r02.sh OUT -- everything is written under OUT (tools/postprocess_r02.sh reads it)
mkdir -p "${1:?output directory}"
F=$(cd "$1" && pwd)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
python bench.py --full > $F/bench_n1.json 2> $F/bench_n1.err || exit 1
python bench.py --full --no-graph --no-f32 --no-cpu-baseline > $F/bench_plan.json 2>/dev/null || exit 1
rocprofv3 --kernel-trace --stats -d $F/prof_bench -o bench -- python3 bench.py --full --steps 50 --warmup 10 --no-f32 --no-cpu-baseline --sustain-seconds 0 > $F/prof_bench.log 2>&1 || exit 1
rocprofv3 --pmc FETCH_SIZE -d $F/pmc_fetch -o f -- python3 bench.py --full --steps 3 --warmup 2 --no-graph --no-f32 --no-cpu-baseline --sustain-seconds 0 > $F/pmc_fetch.log 2>&1 || exit 1
rocprofv3 --pmc WRITE_SIZE -d $F/pmc_write -o w -- python3 bench.py --full --steps 3 --warmup 2 --no-graph --no-f32 --no-cpu-baseline --sustain-seconds 0 > $F/pmc_write.log 2>&1 || exit 1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_MFMA SQ_WAVE_CYCLES SQ_BUSY_CYCLES -d $F/pmc_mfma -o m -- python3 tools/gemm_bench.py --iters 3 > $F/pmc_mfma.log 2>&1 || exit 1
rocprofv3 --pmc SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VALU SQ_INSTS_LDS -d $F/pmc_lds -o l -- python3 tools/gemm_bench.py --iters 3 > $F/pmc_lds.log 2>&1 || exit 1
python tools/gemm_bench.py > $F/gemm_microbench.txt 2>&1
python tools/gemm_bench.py --s1 > $F/s1_gemm_microbench.txt 2>&1
python tools/gemm_bench.py --mx8 > $F/mx8_microbench.txt 2>&1
ls $F
