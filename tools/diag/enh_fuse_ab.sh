set -eo pipefail
for m in 2 1 2 1; do
  python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-exact --mode enh_fuse=$m | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
sh=d['kernel_time_shares']
print('enh_fuse=$m value %.1f'%d['value'], {k[:28]:v for k,v in sh.items() if 'enh' in k or 'gemm' in k or 'warp' in k})"
done
