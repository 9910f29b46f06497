#!/bin/bash
# per-site update timers of the GRU+BPTT config:  tools/gru_sites.sh [ENV=val ...]
env "$@" timeout 500 python bench.py --full --workload gru_bptt --steps 6 --warmup 2 --sustain-steps 0 --no-configs --no-secondary --no-cpu-baseline 2>/dev/null | tail -1 | python -c '
import json,sys
d=json.loads(sys.stdin.read()); f=json.load(open(d["full_report"]))
ls=f.get("update_launch_sites_ms") or {}
print(sys.argv[1], d["value"], d["rollout_ms"], d["update_ms"], " ".join("%s=%.3f" % (k, v["avg_ms"]) for k,v in ls.items() if k.startswith("conv") and "data" in k))' "$*"
