# A/B of the two pre-split GEMM tiles: micro-benchmark, then the 4-lane headline with each variant forced (EG_GEMM_TILE)
# usage: tools/ab_gemm_tiles.sh OUTDIR
set -x
O=${1:?usage: tools/ab_gemm_tiles.sh OUTDIR}
mkdir -p "$O"
python -m pytest tests/test_gpu_kernels.py -x -q -m gpu -k "presplit" 2>&1 | tail -3
python tools/bench_ops.py gemm bf16x3 > "$O/gemm_tiles.txt" 2>&1; cat "$O/gemm_tiles.txt"
for t in 64 128 64 128; do
  EG_GEMM_TILE=$t python bench.py --full --no-train-legs --no-extra-legs --no-cpu-baseline --steps 40 > "$O/bench_tile_$t.json" 2>/dev/null
  python - <<PY
import json
d=json.load(open("$O/bench_tile_$t.json"))
print("TILE $t", d["value"], d["ms_per_step"], d["pose_rel_l2_vs_cpu_oracle"], d["roofline"]["by_kernel_ms_per_step"]["gemm_presplit_kernel (pre-split X)"])
PY
done
for n in 1 2 6 8; do
  python bench.py --no-train-legs --no-extra-legs --no-cpu-baseline --no-roofline --steps 40 --in-flight $n 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('IN-FLIGHT $n', d['value'], d['ms_per_step'])"
done
