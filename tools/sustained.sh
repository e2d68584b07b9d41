# The bench step 50,000 times back to back (no extras): sustained rate, per-launch spread.
# On an MI355X: bash tools/sustained.sh [OUT_DIR]  (writes OUT_DIR, default out/sustained; a heartbeat file while it runs)
O=${1:-out/sustained}
mkdir -p $O || exit 1
python -c "import torch; print('torch', torch.__version__, flush=True)" || exit 1
( for i in $(seq 1 22); do sleep 20; echo "bench running $((i*20)) s" >> $O/heartbeat.txt; done ) &
hb=$!
timeout -k 10 420 python -u bench.py --full --steps 50000 --warmup 100 --no-cpu-baseline --no-extras --configs3-steps 20 > $O/bench_50k.json 2> $O/bench_50k.err
rc=$?
kill $hb 2>/dev/null
tail -c 400 $O/bench_50k.json
exit $rc
