#!/bin/bash
# Round 6: the --full bench (the default run of round 6) three times back to back (run-to-run spread of roofline.frac, wall time per section)
set -uo pipefail
cd "${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
O=${BENCH_OUT:-${TMPDIR:-/tmp}/r6_bench}   # where the lines, full records and logs go
mkdir -p "$O"
tag=${1:-a}
shift || true
for i in 1 2 3; do
  t0=$(date +%s.%N)
  LARVA_BENCH_FULL=$O/r6_bench_full_${tag}$i.json python bench.py --full --steps 20 --warmup 5 "$@" > $O/r6_bench_${tag}$i.json 2> $O/r6_bench_${tag}$i.err || { echo "run $i failed"; tail -20 $O/r6_bench_${tag}$i.err; exit 1; }
  t1=$(date +%s.%N)
  echo "run $i: wall $(python3 -c "print(round($t1 - $t0, 1))") s, line $(wc -c < $O/r6_bench_${tag}$i.json) bytes"
  cat $O/r6_bench_${tag}$i.json
done
