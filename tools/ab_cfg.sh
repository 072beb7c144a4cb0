#!/bin/bash
# A/B of library builds (NGS_LIB variants; "main" = lib/libngram_search.so) over bench configs, one
# pass each in turn, on one GPU box. usage (GPU box, repo root): tools/ab_cfg.sh "<variants>" "<configs>" [steps]
# The bench lines go to $NGS_OUT/ab (default out/ab).
set -o pipefail
VARS=$1; CFGS=$2; STEPS=${3:-50}
O=${NGS_OUT:-out}/ab
mkdir -p $O
for c in $CFGS; do
  for v in $VARS; do
    [ "$v" = main ] && lib="" || lib=$v
    NGS_LIB=$lib timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --no-dropin --config $c --steps $STEPS --warmup 10 > $O/$v.$c.json 2> $O/$v.$c.err || { echo "$v $c failed"; tail -3 $O/$v.$c.err; exit 1; }
    python3 -c "import json; d=json.load(open('$O/$v.$c.json')); print(f\"$c $v: {d['value']:.4f} Mq/s  {d['ms_per_step']:.3f} ms/step  tier1 {d['roofline']['kernel_ms']:.3f} ms  frac {d['roofline']['frac']:.3f} paths {d['detail']['paths']}\")"
  done
done
