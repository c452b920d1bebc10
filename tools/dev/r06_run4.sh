#!/bin/bash
# by-shape timing with / without the slab kernel + step A/B
set -x
out=${OUT_DIR:?set OUT_DIR to the output folder}/r06; mkdir -p $out

MMD_PROF_DUMP=$out/shape_slab.csv python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $out/bench_slab.json 2> $out/bench_slab.err || exit 1
MMD_NO_SLAB=1 MMD_PROF_DUMP=$out/shape_noslab.csv python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $out/bench_noslab.json 2> $out/bench_noslab.err || exit 1
python tools/dev/prof_by_shape.py $out/shape_slab.csv 1 400 > $out/by_shape_slab.txt
python tools/dev/prof_by_shape.py $out/shape_noslab.csv 1 400 > $out/by_shape_noslab.txt
grep -a "f12\|f7 " $out/by_shape_slab.txt | head -12
echo ---; grep -a "f12\|f7 " $out/by_shape_noslab.txt | head -12
bash tools/dev/ab_env.sh MMD_NO_SLAB "1 unset" 3 2>&1 | grep timed
