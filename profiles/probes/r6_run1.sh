set -u
export OUT=${OUT:-r6a}  # output directory
mkdir -p $OUT
export TMPDIR=/tmp
timeout 600 python tests/union_stream_probe.py 1 2 3 > $OUT/union_probe.txt 2>&1; echo "union probe rc=$?"; tail -5 $OUT/union_probe.txt
timeout 300 python tests/and_stream_probe.py 1 2 > $OUT/and_probe.txt 2>&1; echo "and probe rc=$?"; tail -3 $OUT/and_probe.txt
for op in wand maxscore and; do
  timeout 400 python bench.py --full --op $op --steps 30 --warmup 3 > $OUT/bench_$op.json 2> $OUT/bench_$op.err; echo "bench $op rc=$?"; tail -c 600 $OUT/bench_$op.json | head -c 300; echo
done
DS2I_NO_UNION_RSTREAM=1 timeout 400 python bench.py --full --op wand --no-oracle --steps 30 --warmup 3 > $OUT/bench_wand_old.json 2> $OUT/bench_wand_old.err
python - <<'PY'
import json, os
for n in ["wand","maxscore","and","wand_old"]:
    try:
        d=json.loads(open(os.path.join(os.environ['OUT'], 'bench_%s.json')%n).read().strip().splitlines()[-1])
        print(n, round(d["value"]), "q/s", round(d["ms_per_step"],3), "ms/step")
        for k in d["roofline"].get("per_kernel",[]): print("   ", k["kernel"], k["class"], k["queries"], round(k["ms_per_launch"],3))
    except Exception as e: print(n, "FAILED", e)
PY
