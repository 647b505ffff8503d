#!/bin/bash
# GPU box: same-device A/B of one source file: tools/ab_file.sh <csrc file> <alternative file> [bench args]
# builds with the alternative, runs the bench stages, builds with the product file, runs them again; twice.
cd "$(dirname "$0")/.."
CS=bundle-adjusting-gaussian-splatting_amd/csrc
F=$1; ALT=$2; shift 2
run() {
  timeout -k 10 150 python bench.py --full --no-cpu-baseline --no-aabb-leg --steps ${STEPS:-40} --warmup 5 "$@" 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read()); s=d['stage_ms']
print('  ms/step %.4f  stages:'%(d['ms_per_step']), s)"
}
cp $CS/$F /tmp/product_file
for rep in 1 2; do
  cp $ALT $CS/$F; make -C $CS -j8 > /tmp/build.log 2>&1 || { echo "BUILD FAILED"; tail -5 /tmp/build.log; cp /tmp/product_file $CS/$F; exit 1; }
  echo "== alternative (rep $rep)"; run "$@"
  cp /tmp/product_file $CS/$F; make -C $CS -j8 > /tmp/build.log 2>&1 || { echo "BUILD FAILED"; tail -5 /tmp/build.log; exit 1; }
  echo "== product (rep $rep)"; run "$@"
done
