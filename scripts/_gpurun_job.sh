#!/bin/bash
# GPU box: the GPU test suite, smoke(), the --full bench line and the headline kernel profile.  Logs of the first three go under the
# directory given as $1; scripts/profile_job.sh picks the kernel profile's folder itself.
[ -n "$1" ] || { echo "usage: $0 <output dir>" >&2; exit 2; }
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1" && O=$(cd "$1" && pwd) && cd "$R" || exit 1

step() {   # step <name> <seconds> <cmd...>: the command under its own time limit, output in $O/<name>.log
  local name=$1 secs=$2; shift 2
  timeout -k 10 "$secs" "$@" > "$O/$name.log" 2>&1
  local rc=$?
  echo "$name rc=$rc"
  # 0 = passed, 1 = failed checks; anything else (a fault, an abort, a segfault, a time limit) ends the script: nothing more on the GPU
  [ $rc -le 1 ] || { tail -20 "$O/$name.log"; exit $rc; }
}

step gputest 1000 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider
grep -E "passed|failed|^FAILED|^ERROR" "$O/gputest.log" | tail -12
step smoke 300 python -c "import __graft_entry__ as g; g.smoke()"
tail -2 "$O/smoke.log"
step bench 900 python bench.py --full
grep '^{"metric"' "$O/bench.log" | tail -1 > "$O/bench_default.json"
O="$O" python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['O'], 'bench_default.json')).read())
print(d['value'], d['ms_per_step'], d['dtype'], d['step_ms']); print(d['parity']); print(d['cpu_baseline'])
for k in ('fp16_speed', 'parity_mode', 'stego_fast', 'backbone_b32', 'dinov2_fp8'):
    if k in d:
        print(k, d[k]['value'], d[k]['ms_per_step'], d[k]['roofline'].get('frac'), d[k].get('parity'))
print('roofline', d['roofline'])
PY
step profile 900 bash scripts/profile_job.sh r05d_headline 0
cat "$O/profile.log"
