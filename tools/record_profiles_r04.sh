#!/bin/bash
# GPU box: what profiles/ cites for round 4's final build.  Usage: tools/record_profiles_r04.sh <tag> <output dir>  -> <output dir>/<tag>_*
tag=${1:-r04_final}
R=$GRAFT_REPO_ROOT; cd $R
mkdir -p "${2:?output directory}"; O=$(cd "$2" && pwd)
python3 bench.py --full > $O/${tag}_bench.json 2> $O/${tag}_bench.err
for cfg in cfg5 cfg3b cfg2; do python3 bench.py --full --config $cfg --steps 20 --cpu-seconds 4 > $O/${tag}_bench_$cfg.json 2> $O/${tag}_bench_$cfg.err; done
python3 bench.py --full --per-env-wind --steps 20 --no-cpu-baseline --no-env-leg 2>/dev/null | grep "^{" > $O/${tag}_bench_cfg4_per_env_wind.json
PMC_KERNEL="wf_step_ll_kernel<2, 2" bash tools/quick_pmc.sh ${tag} > /dev/null 2>&1
PMC_KERNEL="wf_step_ll_kernel<4, 2, false, false" bash tools/quick_pmc.sh ${tag}_fly --per-env-wind > /dev/null 2>&1
(python3 tools/resolve_cost.py HornsRev1_ 65536; python3 tools/resolve_cost.py HornsRev2_ 131072) 2>&1 | grep -v amdgpu.ids > $O/${tag}_resolve_cost.txt
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_rocprof -- python3 $R/bench.py --no-cpu-baseline --no-env-leg > $O/${tag}_bench_under_rocprof.json 2> $O/${tag}_rocprof.err
cd $R
f=$(find $O/${tag}_rocprof -name "*kernel_stats.csv" | head -1)
python3 tools/summarize_rocprof.py $f $O/${tag}_kernel_stats_bench_cfg4.csv > /dev/null
rm -rf $O/${tag}_rocprof
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${tag}_rocprof -- python3 $R/bench.py --no-cpu-baseline --no-env-leg --per-env-wind > /dev/null 2> $O/${tag}_rocprof_fly.err
cd $R
f=$(find $O/${tag}_rocprof -name "*kernel_stats.csv" | head -1)
python3 tools/summarize_rocprof.py $f $O/${tag}_kernel_stats_bench_cfg4_on_the_fly.csv > /dev/null
rm -rf $O/${tag}_rocprof
ls -la $O/${tag}_*
