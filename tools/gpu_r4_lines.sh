#!/bin/bash
# round 4: the bench lines that are priced with committed counter summaries, re-taken once the summaries of the FINAL library are in the tree
# (configs[2..4] at the sizes of their summaries, the Cornell box and config 5 at their own sizes, the N > 1 rehearsal lines)
set -e
OUT=${OUT:-bench_out}   # where the lines and logs are written
mkdir -p $OUT
python bench.py --full --workload book2_moving --steps 5 --warmup 1 > $OUT/r04_line_book2_moving.json 2> $OUT/r04_line_book2_moving.err
python bench.py --full --workload cornell_box --spp 1000 --steps 5 --warmup 1 > $OUT/r04_line_cornell_box.json 2> $OUT/r04_line_cornell_box.err
python bench.py --full --workload cornell_box --steps 2 --warmup 1 --cpu-seconds 5 > $OUT/r04_line_cornell_box_5000spp.json 2> $OUT/r04_line_cornell_box_5000spp.err
python bench.py --full --workload book2_final --spp 64 --steps 5 --warmup 1 > $OUT/r04_line_book2_final.json 2> $OUT/r04_line_book2_final.err
timeout -k 10 500 python bench.py --full --workload book2_final --steps 1 --warmup 0 --cpu-seconds 10 > $OUT/r04_config5_full.json 2> $OUT/r04_config5_full.err
for n in 2 4; do
  python bench.py --full --gpus $n --backend gloo --same-device --steps 3 --warmup 1 2> $OUT/r04_rehearsal_n$n.err | grep '^{' > $OUT/r04_rehearsal_n$n.json
done
python bench.py --full --steps 20 --warmup 5 > $OUT/r04_headline_again.json 2> $OUT/r04_headline_again.err
cat $OUT/r04_line_*.json $OUT/r04_config5_full.json $OUT/r04_rehearsal_n*.json $OUT/r04_headline_again.json | cut -c1-160
