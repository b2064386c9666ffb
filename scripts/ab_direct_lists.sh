#!/bin/bash
# A/B of a change against its parent (direct lists, PERFLOG row 178; direct
# resolve, row 179): six alternated runs of the plain bench, three with A first
# and three with B first, A = libmcpt_a.so, the parent commit's build
# (scripts/build_base.sh), B = libmcpt.so.  The first pair also dumps image and
# ray count, compared at the end.  Any failing run ends the script.  Output
# under $OUT.
#   bash scripts/build_base.sh libmcpt_a.so
#   bash scripts/ab_direct_lists.sh
set -e -o pipefail
O=${OUT:-build/ab_direct}; mkdir -p $O
L=$PWD/montecarlopathtracer_amd/lib
run() {   # side round [extra bench args]
  local side=$1 r=$2; shift 2
  local lib=libmcpt.so; [ $side = A ] && lib=libmcpt_a.so
  MCPT_LIB_PATH=$L/$lib timeout -k 10 240 python bench.py --gpus 1 --steps ${STEPS:-20} --warmup ${WARMUP:-5} "$@" \
    > $O/${side}_$r.log 2>&1
  echo "round $r $side: $(grep -o '"ms_per_step": [0-9.]*' $O/${side}_$r.log) $(grep -o '"rays_per_step": [0-9]*' $O/${side}_$r.log)"
}
for r in 1 2 3 4 5 6; do
  if [ $((r % 2)) = 1 ]; then first=A; second=B; else first=B; second=A; fi
  dump=""; [ $r = 1 ] && dump=1
  run $first $r ${dump:+--dump-outputs $O/dump_$first}
  run $second $r ${dump:+--dump-outputs $O/dump_$second}
done
python3 - $O <<'PY'
import glob, json, sys
import numpy as np
o = sys.argv[1]
ms = {s: [[json.loads(x) for x in open(f) if x.startswith("{")][-1]["ms_per_step"] for f in sorted(glob.glob(f"{o}/{s}_*.log"))]
      for s in "AB"}
a, b = np.array(ms["A"]), np.array(ms["B"])
print("A ms/frame", a, "mean %.2f spread %.2f" % (a.mean(), a.max() - a.min()))
print("B ms/frame", b, "mean %.2f spread %.2f" % (b.mean(), b.max() - b.min()))
print("B vs A: %+.2f%%; every B below every A: %s" % (100 * (b.mean() / a.mean() - 1), bool(b.max() < a.min())))
same = True
for f in sorted(glob.glob(f"{o}/dump_A/*")):
    g = f.replace("dump_A", "dump_B")
    eq = open(f, "rb").read() == open(g, "rb").read()
    same &= eq
    print("dump", f.split("/")[-1], "identical" if eq else "DIFFERS")
sys.exit(0 if same else 1)
PY
