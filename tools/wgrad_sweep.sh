#!/bin/bash
# sweep the workgroup target of the conv3x3 weight gradient (bench.py --full's instrumented pass, all shapes of the step)
# outputs under $OUT (default sweep_out/)
OUT=${OUT:-sweep_out}; mkdir -p "$OUT"
for wgs in 512 1024 2048 4096; do
  DGTD_WGRAD_WGS=$wgs python bench.py --full --steps 6 --warmup 3 --graph off --no-miou --no-cpu-baseline --all-kernels "$OUT/kernels_sweep.json" > "$OUT/b_sweep.json" 2> "$OUT/b_sweep.err"
  python - "$wgs" "$OUT/kernels_sweep.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))["kernels"]
print("wgs =", sys.argv[1], " ".join(f"{k['kernel'].split('[')[1][:-1]}:{k['avg_us']}" for k in d if "conv3x3_wgrad" in k["kernel"]), flush=True)
PY
done
