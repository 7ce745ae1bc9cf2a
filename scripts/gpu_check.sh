#!/bin/bash
# One GPU-box session: parity tests, soak, smoke, the full bench line, the config-3 harness.  Outputs under $OUT (default out/check).
set -u
O=${OUT:-out/check}
mkdir -p $O
export TMPDIR=/tmp
echo "== pytest -m gpu"
timeout 2400 python -m pytest tests -q -m gpu --durations=5 2>&1 | grep -v amdgpu.ids | tail -14 | tee $O/pytest_gpu.log
echo "== soak"; SOAK_CASES=${SOAK_CASES:-400} timeout 1500 python scripts/soak_parity.py 2>&1 | tail -1 | tee $O/soak.log
echo "== smoke"
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids | tail -2 | tee $O/smoke.log
echo "== bench (full line, CPU baselines included)"
timeout 900 python bench.py --full --steps 20 --warmup 5 2>$O/bench_default.err | tail -1 | tee $O/bench_default.log
grep -v amdgpu.ids $O/bench_default.err | tail -6
echo "== config-3 harness (300 images, then one GPU's share of 38)"
timeout 600 python scripts/config3_harness.py 2>&1 | grep -v amdgpu.ids | tail -1 | tee $O/config3.log
timeout 600 python scripts/config3_harness.py --images 38 --no-graph 2>&1 | grep -v amdgpu.ids | tail -1 | tee $O/config3_38.log
