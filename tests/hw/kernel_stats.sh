#!/bin/bash
# usage: kernel_stats.sh <tag> <bench_configs plan> [out dir]   e.g. cfg5 cfg5:16
# rocprofv3 --kernel-trace --stats of one extras config; the per-kernel table
# goes to <out dir>/<tag>_kernel_stats.md (profiles/db_stats.py); the out dir
# is absolute or relative to the repo root, default profile_out
tag=$1; plan=$2
R=$(cd "$(dirname "$0")/../.." && pwd)
o=$(cd $R && mkdir -p ${3:-profile_out} && cd ${3:-profile_out} && pwd)
cd /tmp && export TMPDIR=/tmp
out=$o/prof_$tag
rm -rf $out
timeout 900 rocprofv3 --kernel-trace --stats -d $out -o p -- python $R/bench_configs.py --plan $plan > $o/${tag}_run.txt 2>&1
db=$(find $out -name "*.db" | head -1)
python $R/profiles/db_stats.py $db > $o/${tag}_kernel_stats.md
head -20 $o/${tag}_kernel_stats.md
rm -rf $out
