#!/bin/bash
# Per-rank work of an N-way band split measured on one GPU (--shard 0/N, rank 0 has the most bands),
# with rank 0's exchange work (--dist), and C2 frames in flight.  Outputs in $BENCH_OUT (default bench_out/).
out=${BENCH_OUT:-bench_out}
mkdir -p "$out"
for n in 2 4 8; do timeout -k 10 120 python bench.py --full --shard 0/$n --no-cpu-baseline --no-roofline --steps 3000 > $out/shard_$n.json 2> $out/shard_$n.err || exit $?; done
timeout -k 10 120 python bench.py --full --dist --shard 0/8 --no-cpu-baseline --no-roofline --steps 3000 > $out/shard_8d.json 2> $out/shard_8d.err || exit $?
timeout -k 10 120 python bench.py --full --config c4 --shard 0/8 --no-cpu-baseline --no-roofline --steps 1000 > $out/shard_c4_8.json 2> $out/shard_c4_8.err || exit $?
for f in 2 4 8; do timeout -k 10 120 python bench.py --full --config c2 --inflight $f --no-cpu-baseline --no-roofline --steps 3000 > $out/c2_inflight_$f.json 2> $out/c2_inflight_$f.err || exit $?; done
