# The round's committed evidence, produced in one call on the GPU box: the driver's command, a longer timed region, and the
# rocprofv3 --kernel-trace --stats summaries of the headline workload and of the three configs[] workloads.
#   bash tools/final_profiles.sh OUTDIR
set -x
R=$(cd "$(dirname "$0")/.." && pwd); mkdir -p "${1:?usage: tools/final_profiles.sh OUTDIR}"; OUT=$(cd "$1" && pwd)
cd $R
python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/round4_bench_n1.json 2> $OUT/round4_bench_n1.err
python bench.py --full --gpus 1 --steps 128 --warmup 8 --configs none > $OUT/round4_bench_n1_128.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp
prof() { tag=$1; shift; rm -rf $OUT/prof_$tag; rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$tag -- python3 $R/bench.py "$@" > $OUT/prof_$tag.log 2>&1; cp $(ls $OUT/prof_$tag/*/*kernel_stats.csv | head -1) $OUT/round4_bench_${tag}_kernel_stats.csv; }
prof f16 --full --gpus 1 --steps 20 --warmup 5 --configs none
prof q4km --child --full --configs none --gpus 1 --steps 64 --warmup 8 --context 512 --sample-tokens 0 --profile-steps 3 --model llama-3.2-3b --quant q4_k_m --cpu-tokens 4
prof 1b --child --full --configs none --gpus 1 --steps 64 --warmup 8 --context 512 --sample-tokens 0 --profile-steps 3 --model llama-3.2-1b --quant f16 --cpu-tokens 16
prof 8bstage --child --full --configs none --gpus 1 --steps 64 --warmup 8 --context 512 --sample-tokens 0 --profile-steps 3 --model llama-3.1-8b --quant q4_k_m --stage-blocks 28:32 --cpu-tokens 8
rm -rf $OUT/prof_f16 $OUT/prof_q4km $OUT/prof_1b $OUT/prof_8bstage
ls -la $OUT/round4_bench_*
