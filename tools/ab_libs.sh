# A/B timing of library builds under ab_tmp/ (ALGP_LIB selects the build; "base" = the product library): the headline run, short
# (--full: the one-stream leg behind serial_kernel_frac).  Lines go to $AB_OUT (default ab_tmp/).
AB_OUT=${AB_OUT:-ab_tmp}
mkdir -p $AB_OUT
for v in "$@"; do
  if [ "$v" = base ]; then unset ALGP_LIB; else export ALGP_LIB=$PWD/ab_tmp/lib_v$v.so; fi
  python3 bench.py --full --no-extras --no-cpu-baseline --steps 10 --warmup 3 > $AB_OUT/ab_$v.json 2> $AB_OUT/ab_$v.err
  python3 -c "
import json,sys
o=json.loads(open('$AB_OUT/ab_$v.json').read().strip().splitlines()[-1])
r=o['roofline']
print('v$v', round(o['ms_per_step'],2), 'frac', round(r['frac'],4), 'avg launch ms', round(r.get('avg_launch_ms',0),4), 'serial', r.get('serial_kernel_frac'))"
done
