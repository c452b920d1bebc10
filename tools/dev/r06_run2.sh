#!/bin/bash
# round 6, second GPU call: slab-kernel parity, by-shape timing with / without it, step A/B, train soak with tuned teachers, launcher at 4 ranks
set -x
out=${OUT_DIR:?set OUT_DIR to the output folder}/r06; mkdir -p $out
timeout -k 10 900 python -m pytest tests/test_gpu_kernels.py -x -q -k "slab or pwconv" > $out/t_slab.log 2>&1; rc=$?
tail -15 $out/t_slab.log
[ $rc -eq 0 ] || exit $rc
# by-shape (hipEvents around every launch of one eager single-stream step): with and without the slab kernel
MMD_PROF_DUMP=$out/shape_slab.csv python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $out/bench_slab.json 2> $out/bench_slab.err || exit 1
MMD_NO_SLAB=1 MMD_PROF_DUMP=$out/shape_noslab.csv python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $out/bench_noslab.json 2> $out/bench_noslab.err || exit 1
python tools/dev/prof_by_shape.py $out/shape_slab.csv 1 400 > $out/by_shape_slab.txt
python tools/dev/prof_by_shape.py $out/shape_noslab.csv 1 400 > $out/by_shape_noslab.txt
grep -a "f12\|f7 " $out/by_shape_slab.txt | head -20
echo ---; grep -a "f12\|f7 " $out/by_shape_noslab.txt | head -20
bash tools/dev/ab_env.sh MMD_NO_SLAB "1 unset" 3 > $out/ab_slab.txt 2>&1; cat $out/ab_slab.txt
