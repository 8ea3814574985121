#!/bin/bash
# after a change of the default kernel: the whole GPU suite, a fuzz campaign over every variant, and the bench line
set -e
OUT=${OUT:-bench_out}   # where the lines and logs are written
mkdir -p $OUT
python -m pytest tests -m gpu -x -q > $OUT/r04_validate_gpu_tests.log 2>&1 || { tail -30 $OUT/r04_validate_gpu_tests.log; exit 1; }
tail -2 $OUT/r04_validate_gpu_tests.log
timeout -k 10 400 python tools/fuzz_campaign.py --seeds 30000 --first 600000 --variants > $OUT/r04_validate_fuzz.txt 2>&1 || { tail -5 $OUT/r04_validate_fuzz.txt; exit 1; }
tail -1 $OUT/r04_validate_fuzz.txt
python bench.py --full --steps 20 --warmup 5 > $OUT/r04_validate_bench.json 2> $OUT/r04_validate_bench.err || { tail -5 $OUT/r04_validate_bench.err; exit 1; }
cut -c1-300 $OUT/r04_validate_bench.json
