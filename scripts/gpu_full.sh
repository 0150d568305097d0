#!/bin/bash
# Full GPU check: test-suite, the --full bench line, rocprofv3 kernel trace of the same bench command (summaries -> $PGV_OUT_DIR/full/, default out/full/).
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
O="${PGV_OUT_DIR:-out}/full"
mkdir -p "$O"
timeout 1200 python -m pytest tests -m gpu -x -q > "$O/pytest.log" 2>&1
tail -3 "$O/pytest.log"
timeout 900 python bench.py --full --steps 2 --warmup 1 > "$O/bench.json" 2> "$O/bench.err"
tail -c 600 "$O/bench.err"
timeout 900 rocprofv3 --kernel-trace --stats -d "$O/prof" -o bench -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-host-frames --no-latency --no-runner --no-side > "$O/bench_under_rocprof.json" 2> "$O/rocprof.err"
python scripts/rocprof_summary.py "$O/prof/bench_results.db" > "$O/kernel_trace.txt" 2>&1
python scripts/trace_gaps.py "$O/prof/bench_results.db" > "$O/gaps.txt" 2>&1
rm -rf "$O/prof"      # the raw trace is tens of MB: only the summaries are kept
head -12 "$O/kernel_trace.txt" | cut -c1-150
