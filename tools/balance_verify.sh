#!/bin/bash
# What had to be green before MISIFT_BALANCE became the default (r05: profiles/r05_balance_default_ab.txt): the whole GPU suite with
# every context of the session balanced, the A/B of tools/balance_ab.py, and the default bench line both ways.
#   bash tools/balance_verify.sh [out_dir]   -> <out_dir>/balance_*.{log,txt,json} (default build/balance_out)
export MISIFT_TUNABLES=1      # the library reads its launch-shape / path variables only under this switch
out=${1:-build/balance_out}
export TMPDIR=/tmp; mkdir -p "$out"
MISIFT_BALANCE=1 timeout 1500 python -m pytest tests -q -m gpu > "$out/balance_pytest_gpu.log" 2>&1
grep -E "passed|failed|error" "$out/balance_pytest_gpu.log" | tail -3
timeout 120 python tools/balance_ab.py > "$out/balance_ab.txt" 2>&1; cat "$out/balance_ab.txt"
for b in 0 1 0 1; do
  MISIFT_BALANCE=$b timeout 300 python bench.py --full --no-match --no-cpu --no-latency --no-pcie > "$out/balance_bench_$b.json" 2>/dev/null
  python - "$out" "$b" <<'PY'
import json, sys
d = json.loads(open("%s/balance_bench_%s.json" % (sys.argv[1], sys.argv[2])).read().strip().splitlines()[-1])
print("MISIFT_BALANCE=%s" % sys.argv[2], d["value"], d["ms_per_step"], d["roofline"]["frac"], {k: v["ms_per_step"] for k, v in d["kernels"].items()})
PY
done
