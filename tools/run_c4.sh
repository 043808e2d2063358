#!/bin/bash
# verify-tile GPU tests, then a short C4 bench.
set -o pipefail
O=${OUT_DIR:-bench_out}; mkdir -p $O
timeout -k 10 900 python -m pytest tests/test_gpu_txn.py -x -q -m gpu -p no:cacheprovider > $O/pytest_gpu_txn.log 2>&1
rc=$?
tail -30 $O/pytest_gpu_txn.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 900 python bench.py --full --config c4 --steps 5 --warmup 1 > $O/bench_c4.json 2> $O/bench_c4.err || { tail -30 $O/bench_c4.err; exit 1; }
cat $O/bench_c4.json
