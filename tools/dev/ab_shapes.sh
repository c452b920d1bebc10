#!/bin/bash
# by-shape family times for two settings of one environment variable, same box: OUT_DIR=<folder> ab_shapes.sh VAR v1 v2  -> $OUT_DIR/shapes_<v>.txt
var=$1; out=${OUT_DIR:?set OUT_DIR to the output folder}; mkdir -p $out
for v in $2 $3; do
  if [ "$v" = "unset" ]; then unset $var; else export $var=$v; fi
  MMD_PROF_DUMP=$out/shapes_$v.csv python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $out/shapes_$v.json 2> $out/shapes_$v.err || exit 1
  python tools/dev/prof_by_shape.py $out/shapes_$v.csv 1 400 > $out/shapes_$v.txt
done
