# usage: AB_OUT=<output folder> bash tools/gpu_ab.sh <tag> "<cfg list>" "<strategy list>" [pytest -k expr]
set -o pipefail
tag=$1; cfgs=$2; strats=$3; kexpr=$4
out=${AB_OUT:?set AB_OUT to the folder that receives the results}/$tag
mkdir -p $out
if [ -n "$kexpr" ]; then
  timeout -k 10 300 python -u -m pytest tests/test_gpu_parity.py tests/test_sorted_gpu.py -x -q -k "$kexpr" --timeout 120 --timeout-method thread > $out/pytest.txt 2>&1 || { echo PYTEST_FAIL; tail -30 $out/pytest.txt; exit 1; }
  tail -1 $out/pytest.txt
fi
for c in $cfgs; do for s in $strats; do
  timeout -k 10 120 python bench.py --full --config $c --strategy $s --cpu-baseline 0 --steps 20 ${BENCH_EXTRA} > $out/b_${c}_$s.json 2> $out/b_${c}_$s.err || { echo BENCH_FAIL; tail $out/b_${c}_$s.err; exit 1; }
  echo "cfg $c $s: $(python tools/bench_brief.py < $out/b_${c}_$s.json)"
done; done
