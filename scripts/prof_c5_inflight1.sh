cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
export GPU_MAX_HW_QUEUES=16
out=${BENCH_OUT:-bench_out}
mkdir -p "$out"
for c in c5 c5u; do
timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $out/prof_$c -o run --output-format csv -- \
    python3 bench.py --full --config $c --steps 50 --warmup 5 --warmup-seconds 0 --inflight 1 --no-cpu-baseline --no-roofline > $out/prof_$c.log 2>&1 || exit $?
done
