# GPU tests, smoke, the full headline bench and rocprofv3 kernel stats from the
# repository root; outputs under $O (default out/$TAG).
set -o pipefail
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
O=${O:-out/${TAG:-r04c}}; mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/tests.log 2>&1 || { echo "tests rc=$?"; tail -30 $O/tests.log; exit 1; }
tail -1 $O/tests.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { echo "smoke rc=$?"; tail -20 $O/smoke.log; exit 1; }
tail -3 $O/smoke.log
timeout -k 10 400 python3 bench.py --full > $O/bench.json 2> $O/bench.err || { echo "bench rc=$?"; tail -5 $O/bench.err; exit 1; }
python3 -c "import json; d=json.load(open('$O/bench.json')); print('bench', d['value'], d['ms_per_step'], d['roofline']['avg_launch_us'], d['conv_stack']['frac'], d['cpu_baseline']['value'])"
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/stats -o run -f csv -- python3 bench.py --steps 10 --warmup 3 > $O/stats.log 2>&1 || { echo "rocprof rc=$?"; exit 1; }
echo done
