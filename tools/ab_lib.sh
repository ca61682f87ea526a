#!/bin/bash
# A/B of two builds of the library on the box this runs on: tools/ab_lib.sh "<a.so> <b.so> ..." [repeats] [extra bench.py flags]
# ("-" = the in-tree librua_hip.so).  Experiment builds: RUA_BUILD_FLAGS=-D... RUA_BUILD_OUT=<x.so> python -m resunet_a_mltsk_keras_amd.build --force
libs=$1; reps=${2:-2}; shift 2 2>/dev/null
mkdir -p gpurun_out
export AB_LINE=$(mktemp)                                  # the bench line of the current run
for r in $(seq $reps); do for l in $libs; do
  if [ "$l" = "-" ]; then unset RUA_LIB_PATH; else export RUA_LIB_PATH=$PWD/$l; fi
  timeout -k 10 150 python bench.py --full --no-cpu-baseline --no-also --steps 60 --warmup 15 "$@" 2>/dev/null > "$AB_LINE" || { echo "$l failed"; exit 1; }
  python - "$l" <<'PY' | tee -a gpurun_out/ab.log
import json, os, sys
j = json.loads(open(os.environ["AB_LINE"]).read().strip().splitlines()[-1])
k = j["roofline"]["all_mfma_kernels"]
print(sys.argv[1], j["ms_per_step"], j["value"], {n: k[n]["ms_per_step"] for n in k if n.startswith(("conv_dmap", "wgrad_dmap"))}, flush=True)
PY
done; done
