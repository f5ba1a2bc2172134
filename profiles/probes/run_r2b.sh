set -x
export OUT=${OUT:-r2b}  # output directory
mkdir -p $OUT
export TMPDIR=/tmp
timeout 2700 python -m pytest tests -m gpu -x -q --durations=12 > $OUT/pytest.log 2>&1
echo "pytest rc=$?" >> $OUT/pytest.log
tail -25 $OUT/pytest.log
timeout 900 python bench.py --full --workload gov2 --steps 20 --warmup 3 > $OUT/bench_gov2.json 2> $OUT/bench_gov2.err
grep -E "class|upload|Traceback|Error" $OUT/bench_gov2.err | cut -c1-400; python - <<'PY'
import json, os
j=json.load(open(os.path.join(os.environ['OUT'], 'bench_gov2.json')))
print({k:j[k] for k in ('value','ms_per_step','kernel_resident_qps','end_to_end_over_resident')}, j['roofline']['kernel'], j['roofline']['frac'], j['cpu_baseline'] and j['cpu_baseline']['value'])
PY
timeout 600 python bench.py --full --workload c2 --steps 10 --warmup 2 --no-cpu-baseline > $OUT/bench_c2.json 2> $OUT/bench_c2.err
grep -E "class|Traceback|Error" $OUT/bench_c2.err | cut -c1-300; cut -c1-400 $OUT/bench_c2.json
