#!/bin/bash
# A/B of library builds on the bench command: one bench line per library (BUGSEG_LIB), twice each, alternating
#   bash scripts/gpu_ab.sh TAG "libA.so libB.so libA.so@VAR=value" "bench args"   (@: an environment setting)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
T=${1:-ab}; LIBS=${2:-libbugseg.so}; ARGS=${3:-}
O=${OUT_ROOT:-prof_out}/$T     # result lines and logs: $OUT_ROOT/TAG (default prof_out/TAG)
mkdir -p $O
export TMPDIR=/tmp
for rep in 1 2; do
  for spec in $LIBS; do
    l=${spec%%@*}; ev=""; [ "$spec" != "$l" ] && ev=${spec#*@}
    n=$(basename $l .so)${ev:+_$ev}
    # (--full: the per-kernel `kernels` table printed below)
    env $ev BUGSEG_LIB=$PWD/bugcar_image_segmentation_amd/$l timeout -k 10 240 python -u bench.py --full --extras 0 --no-cpu-baseline $ARGS > $O/$n.$rep.json 2> $O/$n.$rep.err || { echo "$n failed"; tail -5 $O/$n.$rep.err; exit 1; }
    python - "$n" $O/$n.$rep.json <<'PY'
import json, sys
r = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print(f"{sys.argv[1]:24s} {r['value']:9.1f} fps {r['ms_per_step']:.3f} ms  " + "  ".join(f"{k}:{v['us_per_launch']}" for k, v in r["kernels"].items()), flush=True)
PY
  done
done
