set -o pipefail
# the --full bench line's single-process children on one GPU (GPU 0 once and
# opened twice); results under $OUT (default build/sp_diag)
OUT=${OUT:-build/sp_diag}
mkdir -p "$OUT"
HM_BENCH_SP_DEVICES=0 timeout -k 10 300 python bench.py --full --steps 1 --warmup 0 --secondary cfg4 --no-cpu-baseline > "$OUT/plain_sp0.json" 2> "$OUT/plain_sp0.err" &&
HM_BENCH_SP_DEVICES=0,0 timeout -k 10 300 python bench.py --full --steps 1 --warmup 0 --secondary cfg4 --no-cpu-baseline > "$OUT/plain_sp00.json" 2> "$OUT/plain_sp00.err"
rc=$?
for f in "$OUT"/*.json; do python -c "
import json,sys; l=json.load(open('$f')); w=l['workloads']['cfg4']; s=l['single_process']; print('$f', 'cfg4', w['value'], 'sp', s.get('value'), s.get('wall_ms'), s.get('kernel_GHs_per_device'), s.get('merge'))"; done
exit $rc
