#!/bin/bash
# the whole round-end check: the whole -m gpu suite, smoke(), then the full bench line (bench.py --full: headline, shipped, GI,
# proxies, render_multi, CPU baseline):   tools/gpu_full.sh TAG   (logs and results under $FRT_RESULTS, default bench_results/)
TAG=${1:-r06}
OUT=${FRT_RESULTS:-bench_results}
set -o pipefail
mkdir -p "$OUT"
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$OUT/pytest_${TAG}_full.log" 2>&1
rc=$?
tail -3 "$OUT/pytest_${TAG}_full.log"
[ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke_${TAG}.txt" 2>&1 || { tail -5 "$OUT/smoke_${TAG}.txt"; exit 1; }
tail -1 "$OUT/smoke_${TAG}.txt"
timeout -k 10 900 python -u bench.py --full > "$OUT/bench_${TAG}.json" 2> "$OUT/bench_${TAG}.err" || { tail -20 "$OUT/bench_${TAG}.err"; exit 1; }
tail -1 "$OUT/bench_${TAG}.json" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('ms', d['ms_per_step'], 'value', d['value'], 'shipped', d.get('shipped', {}).get('ms_per_step'), 'gi', d.get('gi', {}).get('ms_per_step'), 'gi shadow', d.get('gi', {}).get('kernel_ms_per_frame', {}).get('shadow')); print('rm', {k: v for k, v in d.items() if k.startswith('render_multi_wall')}); print('proxy', json.dumps(d.get('scaling_proxy'))[:300])"
