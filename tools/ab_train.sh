# same-device A/B of the default train bench for the libraries in $LIBS (default: production vs lib/libxsd_hip_exp.so)
set -e
LOGS=${LOGS:-tool_logs}; mkdir -p "$LOGS"          # per-run logs
for L in ${LIBS:-libxsd_hip.so libxsd_hip_exp.so libxsd_hip.so}; do
  XSD_LIB=$PWD/xmm-superres-denoise_amd/lib/$L timeout -k 10 300 python bench.py --full --steps 6 --warmup 2 --no-extra --no-cpu-baseline > $LOGS/abt_$L.log 2>&1 || { tail -20 $LOGS/abt_$L.log; exit 1; }
  grep "^{" $LOGS/abt_$L.log | python -c "import sys,json; d=json.loads(sys.stdin.read()); r=d['roofline']; print('$L', round(d['value'],2), round(d['ms_per_step'],1), 'conv', round(r['avg_launch_ms'],3), 'wgrad', round(r['wgrad_kernel']['avg_launch_ms'],3))"
done
