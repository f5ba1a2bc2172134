set -x
export OUT=${OUT:-r2a}  # output directory
mkdir -p $OUT
export TMPDIR=/tmp
timeout 2700 python -m pytest tests -m gpu -x -q --durations=15 > $OUT/pytest.log 2>&1
echo "pytest rc=$?" >> $OUT/pytest.log
tail -30 $OUT/pytest.log
timeout 600 python bench.py --full --workload c2 --steps 10 --warmup 2 > $OUT/bench_c2.json 2> $OUT/bench_c2.err
tail -12 $OUT/bench_c2.err; cat $OUT/bench_c2.json
timeout 900 python bench.py --full --workload gov2 --steps 20 --warmup 3 > $OUT/bench_gov2.json 2> $OUT/bench_gov2.err
tail -14 $OUT/bench_gov2.err; cat $OUT/bench_gov2.json
DS2I_NO_BMW_PRUNE=1 timeout 900 python bench.py --full --workload gov2 --steps 20 --warmup 3 --no-cpu-baseline > $OUT/bench_gov2_noprune.json 2> $OUT/bench_gov2_noprune.err
tail -8 $OUT/bench_gov2_noprune.err; cat $OUT/bench_gov2_noprune.json
