# Round-end rehearsal on the GPU box (from the repo root through gpurun): the GPU test suite, smoke(), the bench.
set -e
OUT=gpurun_out
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/gpu_tests.log 2>&1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
timeout -k 10 300 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err
