# One round of profiling evidence for profiles/ (run through gpurun; program directly after `--`, counters in their own runs).
#   stats : rocprofv3 --kernel-trace --stats              bench.py --full --steps 10 --warmup 3 --bracket-every 1   (3 + 10 timed + 10 second-pass = 23 steps; every step bracketed = single stream, so a small kernel's duration is not stretched by a side-stream kernel sharing the CUs)
#   fetch / write : --pmc FETCH_SIZE / --pmc WRITE_SIZE   bench.py --full --steps 2 --warmup 1    (1 + 2 + 3 = 6 steps; --full: the second pass is part of every profiled run)
#   mfma  : --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE (same short run)
# then:  python tools/prof_summary.py $OUT/prof_stats $OUT/prof_fetch $OUT/prof_write 23 6 r02
#        python tools/prof_mfma.py $OUT/prof_mfma 6 r02
set -e
REPO=$GRAFT_REPO_ROOT
OUT=${OUT:-$REPO/prof_out}      # where the runs write (git-ignored)
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
# one stream in EVERY step of the profiled runs (warm-up and second-pass steps too): with the weight gradients on the side stream a small
# kernel that shares the CUs with one of them is recorded with a stretched duration (bn_bwd_finalize: 5.6 -> 10.3 us average)
export MNY_SIDE_STREAM=0
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_stats -o run -- python3 $REPO/bench.py --full --steps 10 --warmup 3 --bracket-every 1 --no-cpu-baseline --no-nms --full-json > $OUT/prof_stats.json 2> $OUT/prof_stats.err
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/prof_fetch -o run -- python3 $REPO/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-nms > /dev/null 2> $OUT/prof_fetch.err
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/prof_write -o run -- python3 $REPO/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-nms > /dev/null 2> $OUT/prof_write.err
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/prof_mfma -o run -- python3 $REPO/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-nms > /dev/null 2> $OUT/prof_mfma.err
ls -la $OUT/prof_stats $OUT/prof_fetch $OUT/prof_mfma | head -30
