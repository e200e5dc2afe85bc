# full GPU check of the tree: parity suite, smoke, full bench line, kernel trace of the bench (stats).  Usage (GPU box): profiles/final_run.sh [out_dir]
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${1:-$ROOT/run_out/final}" && cd "${1:-$ROOT/run_out/final}" && pwd)
cd $ROOT
python -m pytest tests -m gpu -x -q > $OUT/pytest.log 2>&1; echo "pytest rc=$?" ; tail -2 $OUT/pytest.log
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1; tail -1 $OUT/smoke.log
( time python bench.py --full > $OUT/bench.json 2> $OUT/bench.err ) 2> $OUT/bench.time; tail -3 $OUT/bench.time | head -1
python -c "import json; d=json.loads(open('$OUT/bench.json').read().strip().splitlines()[-1]); print('ms_per_step', d['ms_per_step'], 'value', d['value'], 'roofline', d['roofline']['achieved'], d['roofline']['frac'], 'icp', d['extras']['icp']['device_ms'], 'pipeline', d['extras']['pipeline']['total_ms'], d['extras']['pipeline']['icp_ms'], 'cpu', d['cpu_baseline']['value'])"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof -o v5 -- python $ROOT/bench.py --full --no-cpu-baseline > $OUT/prof.log 2>&1; echo "rocprof rc=$?"
ls $OUT/prof | head
cd $ROOT
python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_driver_flags.json 2>/dev/null
python -c "import json; d=json.loads(open('$OUT/bench_driver_flags.json').read().strip().splitlines()[-1]); print('driver flags: ms_per_step', d['ms_per_step'], 'pipeline', d['extras']['pipeline']['total_ms'], 'icp', d['extras']['icp']['device_ms'])"
