set -o pipefail
for ks in 0 2 3 4 8; do
  AVSE_GEMM_KSPLIT=$ks timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 20 --warmup 5 2>/dev/null \
    | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); s=d['breakdown']['stage_ms']; print($ks, d['ms_per_step'], s['v_conv6'], s['enc_dense'], s['dec_dense1'], s['dec_dense2'])" || exit $?
done
