#!/bin/bash
# Full GPU test suite, then a default bench run (log under $OUT/chk).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
OUT=${OUT:-out}  # where logs and results go
mkdir -p $OUT/chk
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/chk/pytest.log 2>&1 || { tail -40 $OUT/chk/pytest.log; exit 1; }
tail -1 $OUT/chk/pytest.log
timeout -k 10 400 python bench.py --full > $OUT/chk/bench.log 2>&1 || { tail -20 $OUT/chk/bench.log; exit 1; }
tail -1 $OUT/chk/bench.log > $OUT/chk/bench.json
python3 - "$OUT/chk/bench.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
h = d["hbm_fed"]
print("main", round(d["value"], 1), "dec_us", round(d["roofline"]["avg_launch_us"], 1), "frac", round(d["roofline"]["frac"], 3))
print("hbm", round(h["value"], 1), "enc", round(h["encode_us"], 1), "dec", round(h["decode_us"], 1))
print("configs", {k: round(v["value"], 1) for k, v in d.get("configs", {}).items()})
print("host", {k: (v.get("value") if isinstance(v, dict) else v) for k, v in d.get("host_paths", {}).items()})
print("cpu", d.get("cpu_baseline", {}).get("value"), d.get("cpu_baseline", {}).get("kind"))
PY
