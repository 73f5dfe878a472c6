#!/bin/bash
# A/B of where the HIP runtime puts kernel arguments (HIP_FORCE_DEV_KERNARG: unset = the
# runtime's default, 1 = device memory, 0 = host memory), C2 and C3, two reps.  JSON lines in
# $BENCH_OUT/ab/kaV_CONFIG_REP.json (default bench_out/; scripts/ab_table.py DIR reads them).
out=${BENCH_OUT:-bench_out}/ab
mkdir -p "$out"
for r in 1 2; do
  for c in c2 c3; do
    for v in def 1 0; do
      if [ $v = def ]; then
        timeout -k 10 200 python bench.py --full --config $c --no-cpu-baseline --no-roofline --steps 300 > $out/ka${v}_${c}_${r}.json 2> $out/ka${v}_${c}_${r}.err || exit 1
      else
        HIP_FORCE_DEV_KERNARG=$v timeout -k 10 200 python bench.py --full --config $c --no-cpu-baseline --no-roofline --steps 300 > $out/ka${v}_${c}_${r}.json 2> $out/ka${v}_${c}_${r}.err || exit 1
      fi
    done
  done
done
