#!/bin/bash
# on the GPU box: in-situ per-layer profile of the current library -> $OUT/insitu_<tag>/ (OUT defaults to out) ;  tools/insitu_run.sh <tag>
tag=$1
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p $OUT
rocprofv3 --kernel-trace --output-format csv -d $OUT/insitu_$tag -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --profile-json $OUT/insitu_$tag.prof.json > $OUT/insitu_$tag.log 2>&1
tail -1 $OUT/insitu_$tag.log | cut -c1-140
python tools/insitu.py $(ls $OUT/insitu_$tag/*/*kernel_trace.csv) $OUT/insitu_$tag.prof.json --by-shape > $OUT/insitu_$tag.txt
head -9 $OUT/insitu_$tag.txt
