export OUT=${OUT:-r2c}  # output directory
export TMPDIR=/tmp
mkdir -p $OUT
DS2I_DEBUG_PLAN=1 python profiles/probes/class_probe2.py 2>&1 | grep -v amdgpu.ids | grep -v "ds2i plan" | tee $OUT/class_probe2.log
timeout 2700 python -m pytest tests -m gpu -x -q > $OUT/pytest.log 2>&1; tail -5 $OUT/pytest.log
timeout 900 python bench.py --full --workload gov2 --steps 20 --warmup 3 > $OUT/bench_gov2.json 2> $OUT/bench_gov2.err
grep -E "^class|Traceback|Error" $OUT/bench_gov2.err | cut -c1-330; python - <<'PY'
import json, os
j=json.load(open(os.path.join(os.environ['OUT'], 'bench_gov2.json')))
print({k:j[k] for k in ('value','ms_per_step','kernel_resident_qps','end_to_end_over_resident')}, j['roofline']['kernel'], j['roofline']['frac'], j['cpu_baseline'] and j['cpu_baseline']['value'])
PY
