cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
mkdir -p $R/gpurun_out/prof
cd $R
P=$(python3 -c 'import sys; sys.path.insert(0, "scripts"); import summarize_prof; print(summarize_prof.SRC)')  # where summarize_prof.py reads the passes
# --full: the summary keeps this pass's JSON line, whose per-kernel HIP-event times only --full measures
rocprofv3 --kernel-trace --stats --output-format csv -d "$P/kt" -- python3 bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-secondary > "$P/kt.log" 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d gpurun_out/prof/fetch -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > gpurun_out/prof/fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d gpurun_out/prof/write -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > gpurun_out/prof/write.log 2>&1
rocprofv3 -L > gpurun_out/prof/counters.txt 2>&1
find gpurun_out/prof -name "*.csv" | head -30
du -sh gpurun_out/prof
