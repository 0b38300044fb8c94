#!/bin/bash
# PMC passes for the roofline kernel (coset LDE) + a 2^22 bench line.
set -o pipefail
OUT=${LSP_OUT:-bench_out}  # where logs and results go (git-ignored)
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-pmc}
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$TAG/kt -o lde -- python3 tools/lde_probe.py 19 3 > $OUT/$TAG.kt.log 2>&1 || { tail -20 $OUT/$TAG.kt.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/$TAG/fetch -o lde -- python3 tools/lde_probe.py 19 3 > $OUT/$TAG.fetch.log 2>&1 || { tail -20 $OUT/$TAG.fetch.log; exit 1; }
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/$TAG/write -o lde -- python3 tools/lde_probe.py 19 3 > $OUT/$TAG.write.log 2>&1 || { tail -20 $OUT/$TAG.write.log; exit 1; }
echo "pmc done"
timeout -k 10 600 python bench.py --log-n 22 --steps 3 --warmup 1 --full --no-cpu-baseline > $OUT/bench22_$TAG.json 2> $OUT/bench22_$TAG.err || { tail -20 $OUT/bench22_$TAG.err; exit 1; }
cut -c1-600 $OUT/bench22_$TAG.json
timeout -k 10 900 python bench.py --air wide --log-n 20 --steps 2 --warmup 1 --full --no-cpu-baseline > $OUT/bench_wide_$TAG.json 2> $OUT/bench_wide_$TAG.err || { tail -20 $OUT/bench_wide_$TAG.err; exit 1; }
cut -c1-300 $OUT/bench_wide_$TAG.json
