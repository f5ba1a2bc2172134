set -u
OUT=gpurun_out/${1:-r6s}
mkdir -p $OUT
export TMPDIR=/tmp
timeout 900 python tests/ranked_stream_probe.py 1 2 3 > $OUT/ranked_probe.txt 2>&1; echo "ranked probe rc=$?"; tail -4 $OUT/ranked_probe.txt
DS2I_UNIT_CAP=8 timeout 900 python tests/ranked_stream_probe.py 1 > $OUT/ranked_probe_cap.txt 2>&1; echo "ranked probe cap rc=$?"; tail -2 $OUT/ranked_probe_cap.txt
timeout 900 python -m pytest tests/test_gpu.py -x -q -k "topk_beyond_64 or topk_other_k or long_queries" > $OUT/pytest_subset.txt 2>&1; echo "pytest rc=$?"; tail -3 $OUT/pytest_subset.txt
timeout 600 python bench.py --full --workload c2 --k 100 --steps 30 --warmup 3 --no-cpu-baseline > $OUT/bench_c2_k100.json 2> $OUT/bench_c2_k100.err
timeout 600 python bench.py --full --workload c2 --k 1000 --steps 20 --warmup 3 --no-cpu-baseline --no-oracle > $OUT/bench_c2_k1000.json 2> $OUT/bench_c2_k1000.err
timeout 600 python bench.py --full --k 100 --steps 30 --warmup 3 --no-cpu-baseline --no-oracle > $OUT/bench_gov2_k100.json 2> $OUT/bench_gov2_k100.err
python - $OUT <<'PY'
import json,sys,glob
for f in sorted(glob.glob(sys.argv[1]+"/bench_*.json")):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1])
        print(f.split("/")[-1], round(d["value"]), "q/s", round(d["ms_per_step"],3), "ms/step", " ".join("%s=%.2f"%(k["kernel"][-7:],k["ms_per_launch"]) for k in d["roofline"].get("per_kernel",[])))
    except Exception as e: print(f, "FAILED", e)
PY
