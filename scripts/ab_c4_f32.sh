#!/bin/bash
# config 4 / config 2 in Float32 at the head (events)
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
show() { python - "$1" "$2" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
r = d["roofline"]
print("%-10s ms/step %.4f  kernel %s avg %.4f ms median %.4f ms  frac %.3f  check %s" % (sys.argv[1], d["ms_per_step"], r["kernel"][:40], r["avg_launch_ms"], r["median_launch_ms"], r["frac"], d.get("result_check", {}).get("ok")))
PY
}
for rep in 1 2; do
python bench.py --full --config c4 --dtype f32 --soak-seconds 0 --no-cpu-baseline --no-plain-handover > $OUT/ab_c4f32.json 2>/dev/null; show c4_f32 $OUT/ab_c4f32.json
for v in "$@"; do
  scripts/with_variant.sh $v python bench.py --full --config c4 --dtype f32 --soak-seconds 0 --no-cpu-baseline --no-plain-handover > $OUT/ab_$v.json 2>/dev/null; show $v $OUT/ab_$v.json
done
done
