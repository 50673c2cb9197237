#!/bin/bash
# same-box A/B of environment switches on the default fused step: tools/gpu_ab.sh "A=1" "B=2 C=3" ...   (an empty string = the default)
# The bench lines go to $OUT (default tools/tmp).  Each run has its own time limit; the first run that fails ends the whole A/B.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-tools/tmp}
mkdir -p "$OUT"
i=0
for rep in 1 2; do
for e in "$@"; do
  i=$((i+1))
  env $e timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-extras --no-cpu-baseline --graph off > "$OUT/sw_$i.json" 2> "$OUT/sw_$i.err"
  rc=$?
  if [ $rc -ne 0 ]; then
    echo "[$e] bench.py failed (exit $rc); stopping the A/B here" >&2
    tail -5 "$OUT/sw_$i.err" >&2
    exit $rc
  fi
  python - "$e" "$OUT/sw_$i.json" <<'PY'
import json, sys
try:
    d = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
    pc = d["roofline"]["per_class"]
    print("[%s]" % sys.argv[1], round(d["value"]), round(d["ms_per_step"], 3), "serial", round(d["work_per_step"]["ms_per_step_profiled_serial"], 3), " ".join("%s=%.3f" % (k, v["ms_per_step"]) for k, v in pc.items() if v["ms_per_step"] > 0.2))
except Exception as ex:
    print("[%s] failed" % sys.argv[1], ex)
PY
done
done
