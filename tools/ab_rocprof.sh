#!/bin/bash
# On the GPU box: kernel-trace stats of a short bench run under an environment switch.   tools/ab_rocprof.sh <tag> VAR=value ...
tag=$1; shift
for kv in "$@"; do export "$kv"; done
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p $OUT          # results directory
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/ab_${tag} -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-conditioning --no-parity --no-roofline > /dev/null 2> $OUT/ab_${tag}.log
cp $(ls $OUT/ab_${tag}/*/*kernel_stats.csv | head -1) $OUT/ab_${tag}_kernel_stats.csv
rm -rf $OUT/ab_${tag}
