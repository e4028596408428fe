# A/B of several experiment builds inside ONE gpurun call: each arg = "<lib suffix>:<env assignments>", e.g.
#   bash scripts/ab_march_libs.sh "_ab:LBMDEM_MARCH=2" "_ab:LBMDEM_MARCH=21" "_ab_x:LBMDEM_MARCH=2"
ROOT=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)   # the repository
cd $GRAFT_REPO_ROOT
P='import sys,json; d=json.loads(sys.stdin.read()); print("MLUPS", d["value"], "ms/step", d["ms_per_step"], "fused_ms", d["collide_stream_kernel_ms"], "frac", d["roofline"]["frac"])'
for rep in 1 2; do
  for a in "$@"; do
    lib=${a%%:*}; e=${a#*:}
    echo "[$lib $e] $(env LBMDEM_HIP_LIBRARY=$ROOT/2d-lbm-dem_amd/liblbmdem_hip$lib.so $e python bench.py --full --steps 40 --warmup 5 --no-cpu-baseline 2>/dev/null | tail -1 | python -c "$P")"
  done
done
