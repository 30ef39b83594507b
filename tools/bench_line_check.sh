# the bench-line tests, smoke, and the default line with --full (roofline, 256^3 kernels, CPU baseline); logs under $TP_CHECK_OUT
export TMPDIR=/tmp
out=${TP_CHECK_OUT:-/tmp/tp_check}
mkdir -p "$out"
timeout 300 python -m pytest tests/test_bench_line.py tests/test_gpu_parity.py -q -m gpu -k "bench or vcycle or golden" 2>&1 | tail -3
timeout 120 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -n 1
timeout 400 python bench.py --full > "$out/bench_final.json" 2> "$out/bench_final.err"
python - "$out/bench_final.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
r = d["roofline"]
print("ms/step %.2f its %s launches %.0f value %.4e" % (d["ms_per_step"], d["config"]["cg_its"], d["config"]["kernel_launches_per_step"], d["value"]))
print("in-step cheb %.1f us frac %.3f (%s) | back-to-back %.1f us frac %.3f | spmv %.1f us frac %.3f" % (1e3 * r["avg_launch_ms"], r["frac"], r["avg_launch_how"], 1e3 * r["back_to_back"]["avg_launch_ms"], r["back_to_back"]["frac"], 1e3 * r["spmv"]["avg_launch_ms"], r["spmv"]["frac"]))
print("256:", r["spmv256"]["spmv"]["frac"], r["spmv256"]["cheb"]["frac"])
print("cpu:", d["cpu_baseline"]["value"], d["cpu_baseline"]["sample"][:160])
PY
