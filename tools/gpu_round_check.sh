# the round's GPU acceptance: full -m gpu suite (no -x: one failure must not hide the rest), smoke, default bench with --full;
# logs under $TP_CHECK_OUT
set -x
export TMPDIR=/tmp
out=${TP_CHECK_OUT:-/tmp/tp_check}
mkdir -p "$out"
timeout 1100 python -m pytest tests -q -m gpu --durations=25 -p no:cacheprovider > "$out/pytest.log" 2>&1; echo "pytest rc=$?" >> "$out/pytest.log"
timeout 120 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out/smoke.log" 2>&1
timeout 600 python bench.py --full > "$out/bench_default.json" 2> "$out/bench_default.err"; echo "bench rc=$?"
tail -n 45 "$out/pytest.log"; tail -n 2 "$out/smoke.log"; cat "$out/bench_default.json"; tail -n 5 "$out/bench_default.err"
