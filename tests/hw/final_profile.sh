#!/bin/bash
# usage: final_profile.sh <tag> [out dir]   (on the GPU box, from the repo root;
# the set goes to <out dir>, relative to the repo root, default profile_out)
# the full bench line (headline, parity gate, PMC traffic by its own child
# runs, CPU baseline, all extras: bench.py --full) -> rocprofv3 kernel stats
# of the same workload and the line that process printed (HIP events vs
# rocprof averages)
tag=$1
R=$PWD
out=$R/${2:-profile_out}
mkdir -p $out
timeout 900 python bench.py --full > $out/bench_$tag.json 2> $out/bench_$tag.log
tail -4 $out/bench_$tag.log; cut -c1-600 $out/bench_$tag.json
cd /tmp && export TMPDIR=/tmp
rm -rf $out/prof_$tag
timeout 600 rocprofv3 --kernel-trace --stats -d $out/prof_$tag -o $tag -- python $R/bench.py --steps 5 --warmup 1 > $out/prof_$tag.log 2>&1
db=$(find $out/prof_$tag -name "*.db" | head -1)
python $R/profiles/db_stats.py $db > $out/kernel_stats_$tag.md; head -8 $out/kernel_stats_$tag.md
grep "^{\"metric" $out/prof_$tag.log > $out/prof_${tag}_bench.json
find $out/prof_$tag -type f -size +4M -delete
# one Encoder::compress / Decoder::decompress call per bench input: the
# product library's rule, then the test build at four long-stream thresholds
cd $R
{ echo "# product library (pieces for inputs of 32 KiB and more that expand by half, and of 256 KiB and more)";
  python tests/hw/scalar_latency.py 2>/dev/null;
  for t in 16384 65536 262144; do echo "# test build, SNAPMI_LONG_STREAM=$t";
    SNAPMI_TESTING=1 SNAPMI_LONG_STREAM=$t python tests/hw/scalar_latency.py 2>/dev/null | cut -c1-76; done; } > $out/scalar_latency_$tag.txt
head -14 $out/scalar_latency_$tag.txt
# kernel trace of one 2 GiB raw stream
bash tests/hw/kernel_stats.sh stream_$tag stream:2 $out > /dev/null 2>&1
grep -E "k_stream|k_decompress_streams3" $out/stream_${tag}_kernel_stats.md | cut -c1-150
grep -h decompress_stream_gibs $out/stream_${tag}_run.txt | cut -c1-250
