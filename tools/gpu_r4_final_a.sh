#!/bin/bash
# round-4 evidence, part A (one gpurun call): the whole GPU suite, the counter summaries + bench lines of all four workloads (default kernel) and of
# the headline under kernel variant 6, the tolerance-mode measurement, bench lines of configs[2..4]
set -e
OUT=${OUT:-bench_out}   # where the lines and logs are written
mkdir -p $OUT
python -m pytest tests -m gpu -x -q > $OUT/r04_final_gpu_tests.log 2>&1 || { tail -30 $OUT/r04_final_gpu_tests.log; exit 1; }
tail -2 $OUT/r04_final_gpu_tests.log
bash tools/gpu_r4_profiles.sh
bash tools/gpu_r4_tol.sh > $OUT/r04_tol.log 2>&1 || { tail -20 $OUT/r04_tol.log; exit 1; }
tail -8 $OUT/r04_tol.log | cut -c1-300
python bench.py --full --workload book2_moving --steps 5 --warmup 1 > $OUT/r04_line_book2_moving.json 2> $OUT/r04_line_book2_moving.err
python bench.py --full --workload cornell_box --spp 1000 --steps 5 --warmup 1 > $OUT/r04_line_cornell_box.json 2> $OUT/r04_line_cornell_box.err
python bench.py --full --workload cornell_box --steps 2 --warmup 1 --cpu-seconds 5 > $OUT/r04_line_cornell_box_5000spp.json 2> $OUT/r04_line_cornell_box_5000spp.err
python bench.py --full --workload book2_final --spp 64 --steps 5 --warmup 1 > $OUT/r04_line_book2_final.json 2> $OUT/r04_line_book2_final.err
cat $OUT/r04_line_*.json | cut -c1-200
