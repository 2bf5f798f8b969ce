#!/bin/bash
# lanes A/B for config 3 fp32 on one box (the fp32 kernels are not power-limited: overlap should come back as time); logs go to OUT_DIR
O=${1:?usage: tools/r05_lanes_f32_ab.sh OUT_DIR}; mkdir -p "$O"
for L in 1 2 3 4 1 2; do
  python bench.py --full --config 3 --dtype f32 --lanes $L --steps 2 --warmup 1 --no-cpu-baseline > "$O"/tmp_f32_l$L.json 2> "$O"/tmp.err || exit 1
  python - "$O" $L <<'PY' | tee -a "$O"/lanes_f32_ab.txt
import json, sys
d = json.loads(open(f"{sys.argv[1]}/tmp_f32_l{sys.argv[2]}.json").read().strip().splitlines()[-1])
print("config3 f32 lanes", sys.argv[2], d["ms_per_step"], "sum of kernels (single-lane profile step)", round(sum(v["ms_total"] for v in d["kernels"].values()), 1))
PY
done
