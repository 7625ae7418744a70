set -o pipefail
cd "${ARX_REPO:-$(dirname "$0")/..}"
O=${ARX_OUT:-out}/r03
mkdir -p $O
TAG=r03k
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/pytest_gpu_$TAG.log 2>&1 || { echo "pytest failed"; tail -30 $O/pytest_gpu_$TAG.log; exit 1; }
tail -3 $O/pytest_gpu_$TAG.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1 || { echo "smoke failed"; tail -20 $O/smoke_$TAG.log; exit 1; }
timeout -k 10 400 python3 bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err || { echo "bench failed"; tail -20 $O/bench_$TAG.err; exit 1; }
cat $O/bench_$TAG.json
