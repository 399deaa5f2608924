#!/bin/bash
# usage: scripts/exp/final_check.sh <out dir>
out=${1:?usage: final_check.sh OUT_DIR}
mkdir -p $out
python -m pytest tests -x -q -m gpu 2>&1 | tail -12 > $out/r06_gpu_tests_final.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids | tail -2 >> $out/r06_gpu_tests_final.txt
python bench.py --full 2>$out/r06_bench_final.err | tail -1 > $out/r06_bench_line_final.json
python bench.py --steps 20 --warmup 5 --full --no-regimes --no-replicas 2>/dev/null | tail -1 > $out/r06_bench_line_final_20.json
cat $out/r06_gpu_tests_final.txt
python - $out <<'PY'
import json, sys
for f in ("r06_bench_line_final.json", "r06_bench_line_final_20.json"):
    d = json.loads(open(sys.argv[1] + "/" + f).read().strip().split("\n")[-1])
    print(f, d["ms_per_step"], "%.4e" % d["value"], d["roofline"]["frac"], d["roofline"]["kernel_us"])
PY
