# quick check of the default build: wgrad/conv kernel tests, then the DN train bench (B=32)
set -e
LOGS=${LOGS:-tool_logs}; mkdir -p "$LOGS"          # per-run logs
timeout -k 10 600 python -m pytest tests/test_hip_kernels.py -x -q -m gpu -k "bf16x6" > $LOGS/q_pytest.log 2>&1 || { tail -30 $LOGS/q_pytest.log; exit 1; }
tail -1 $LOGS/q_pytest.log
fmt='import sys,json
for d in map(json.loads, sys.stdin):
    r=d["roofline"]; print({k:d[k] for k in ("value","ms_per_step")}, "conv ms", round(r["avg_launch_ms"],3), "frac", round(r["frac"],3), "wgrad ms", r.get("wgrad_kernel",{}).get("avg_launch_ms"))'
timeout -k 10 300 python bench.py --full --steps 6 --warmup 2 --no-extra > $LOGS/q_train.log 2>&1
grep "^{" $LOGS/q_train.log | python -c "$fmt"
timeout -k 10 300 python bench.py --full --workload dn_fwd --steps 6 --warmup 2 --no-extra > $LOGS/q_fwd.log 2>&1
grep "^{" $LOGS/q_fwd.log | python -c "$fmt"
