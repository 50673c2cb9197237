#!/bin/bash
# the whole GPU suite + the full bench line (what the driver runs at round end).  Results go to $OUT (default tools/tmp).
# Every GPU step runs under its own time limit; the script stops at the first one that fails.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-tools/tmp}
mkdir -p "$OUT"
timeout -k 10 2400 python -m pytest tests -x -q -m gpu > "$OUT/gputests.txt" 2>&1
rc=$?; echo "rc=$rc" >> "$OUT/gputests.txt"
tail -8 "$OUT/gputests.txt"
[ $rc -eq 0 ] || { echo "gpu_suite: the GPU tests failed (exit $rc); nothing more is started" >&2; exit $rc; }
timeout -k 10 600 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"
rc=$?; tail -c 600 "$OUT/bench_default.err"
[ $rc -eq 0 ] || { echo "gpu_suite: bench.py --full failed (exit $rc)" >&2; exit $rc; }
python - "$OUT/bench_default.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], json.dumps(d.get("extras"))[:1500])
PY
