# tools/final_run.sh OUTDIR — the measurement pass behind profiles/r06_*final* (on an MI355X, from the repo root; results go to OUTDIR):
#   the full bench line (bench.py --full); one `rocprofv3 --kernel-trace --stats` per workload over a steady-only run (balls, sponza, hairball, config 4, config 5), so that every
#   roofline block's kernel time can be recomputed from profiles/r05_rocprofv3_kernel_stats_<scene>.csv; the counter passes; kbench / bigconfigs.
set -x
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${1:?usage: tools/final_run.sh OUTDIR}" && cd "$1" && pwd)
# every GPU step runs under its own time limit; the first one that fails, faults or times out ends the pass
fail() { echo "final_run.sh: stopped, $1 exited with status $2" >&2; exit 1; }
cd $ROOT
R=r06
timeout -k 10 1200 python bench.py --full > $OUT/${R}_bench_final.json 2> $OUT/bench.err || fail bench.py $?
tail -c 400 $OUT/bench.err
cd /tmp; export TMPDIR=/tmp
for s in balls sponza hairball config4 config5; do
  case $s in config5) st=3; wu=1;; config4) st=40; wu=5;; balls) st=400; wu=10;; *) st=100; wu=10;; esac
  rm -rf /tmp/rp_$s
  timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_$s -o b -- python $ROOT/bench.py --scene $s --steps $st --warmup $wu --no-cpu-baseline --no-pmc --no-secondary --steady-only > $OUT/${R}_bench_under_rocprof_$s.json 2>/tmp/rp_$s.err || fail "rocprofv3 bench.py --scene $s" $?
  cp $(find /tmp/rp_$s -name "*kernel_stats.csv" | head -1) $OUT/${R}_rocprofv3_kernel_stats_$s.csv || fail "kernel stats of $s" $?
done
# the device BLAS builder (bvh_device.hip): per-kernel times of two hairball scene creations + one sponza creation
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rpb -o b -- python $ROOT/tools/build_times.py > /tmp/rpb.log 2>&1 || fail "rocprofv3 build_times.py" $?
cp $(find /tmp/rpb -name "*kernel_stats.csv" | head -1) $OUT/${R}_rocprofv3_kernel_stats_scene_build.csv || fail "kernel stats of the scene build" $?
cd $ROOT
NRAYS_BUILD_TIMES=1 timeout -k 10 200 python tools/build_times.py > /tmp/build_times.log 2>&1 || fail build_times.py $?
grep -v "8 triangles\|80 triangles\|192 tri\|amdgpu.ids\|upload of 0.0" /tmp/build_times.log > $OUT/${R}_build_times.log
for s in balls sponza hairball; do
  timeout -k 10 500 python tools/pmc_collect.py $s $OUT/${R}_pmc_$s.json > /tmp/pmc_$s.log 2>&1 || fail "pmc_collect.py $s" $?
done
timeout -k 10 400 python tools/kbench.py --scenes balls,ballsaway,primitives,sponza,sponza8,hairball --steps 30 > $OUT/${R}_kbench_final.log 2>&1 || fail kbench.py $?
timeout -k 10 600 python tools/bigconfigs.py > $OUT/${R}_bigconfigs.log 2>&1 || fail bigconfigs.py $?
timeout -k 10 600 python tools/tile_scaling.py sponza8_4k > /tmp/tile_scaling.log 2>&1 || fail tile_scaling.py $?
grep -v amdgpu.ids /tmp/tile_scaling.log > $OUT/${R}_tile_scaling.log
timeout -k 10 300 python tools/rank_bounds.py > /tmp/rank_bounds.log 2>&1 || fail rank_bounds.py $?
grep world /tmp/rank_bounds.log >> $OUT/${R}_tile_scaling.log
for s in balls primitives sponza sponza8 hairball; do
  timeout -k 10 300 python tools/regimes.py $s > /tmp/regimes_$s.log 2>&1 || fail "regimes.py $s" $?
  grep scene /tmp/regimes_$s.log >> $OUT/${R}_regimes_final.log
done
OUT=$OUT python - <<'PY'
import json, csv, glob, os
out = os.environ['OUT']
d=json.loads(open(out + '/r06_bench_final.json').read().strip().splitlines()[-1])
def show(n, m):
    r=m['roofline']; print(n, m['value'], m['ms_per_step'], r.get('kernel_ms'), r.get('kernel_ms_events'), r['frac'], r['bound'], r.get('dram_frac'), r.get('valu_active_frac'), m.get('cpu_baseline',{}).get('value'), m.get('gpu_over_cpu'), m.get('gpu_over_cpu_at_full_host'))
show('balls', d)
for k,v in d.get('secondary',{}).items():
    if 'roofline' in v: show(k, v)
print(d.get('north_star_sponza'))
for f in sorted(glob.glob(out + '/r06_rocprofv3_kernel_stats_*.csv')):
    rows=[r for r in csv.DictReader(open(f)) if 'k_primary' in r['Name'] or 'k_resolve' in r['Name']]
    print(f.split('stats_')[-1], [(r['Name'][:48], r['Calls'], round(float(r['AverageNs'])/1e3,2)) for r in rows[:3]])
PY
