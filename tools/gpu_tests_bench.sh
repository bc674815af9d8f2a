O=${OUT_DIR:-bench_out}/t; mkdir -p $O
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gpu_tests.log 2>&1
rc=$?; tail -4 $O/gpu_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-e2e > $O/cfg2.json 2> $O/cfg2.err || { tail $O/cfg2.err; exit 1; }
python3 -c "import json;d=json.load(open('$O/cfg2.json'));print(d['ms_per_step'], d['value'], d['verify']['all'], d['stage_ms'])"
