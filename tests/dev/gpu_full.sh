# full GPU validation: test suite, smoke, the full bench (with the CPU baseline and the secondary workloads); the bench line goes to $OUT
OUT=${OUT:-build/bench}
timeout 1400 python -m pytest tests -m gpu -x -q 2>&1 | tail -3
timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
mkdir -p "$OUT"
( time timeout 900 python bench.py --full > "$OUT/bench_full.json" 2> "$OUT/bench_full.err" ) 2>&1 | grep real
tail -c 6000 "$OUT/bench_full.json"
