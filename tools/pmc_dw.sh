# FETCH_SIZE / WRITE_SIZE of the depthwise forward variants (separate --pmc passes over bench.py --full, program directly after `--`)
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/prof_out}      # where the runs write (git-ignored)
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
run() {  # tag, counter
  rocprofv3 --pmc $2 --output-format csv -d $OUT/pmc_$1_$2 -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-nms > /dev/null 2> $OUT/pmc_$1_$2.err
}
run A FETCH_SIZE; run A WRITE_SIZE
export MNY_DW_V1=1; run D FETCH_SIZE; run D WRITE_SIZE; unset MNY_DW_V1
cd $OUT
python3 - <<'PY'
import csv, glob, collections, os, re
for d in sorted(glob.glob('pmc_*_*_SIZE')):
    f = glob.glob(d + '/**/run_counter_collection.csv', recursive=True)
    if not f: print(d, 'no csv'); continue
    tot = collections.defaultdict(float); cnt = collections.Counter()
    for r in csv.DictReader(open(f[0])):
        k = r['Kernel_Name']
        if 'dw3_fwd' in k or 'dw_slide' in k:
            k = re.sub(r'^void mny::', '', k); k = re.sub(r'\(.*', '', k)
            tot[k] += float(r['Counter_Value']); cnt[k] += 1
    for k in sorted(tot): print(os.path.basename(d), k, cnt[k], 'launches', round(tot[k] * 1024 / 3 / 1e9, 3), 'GB/step (raw counter, KiB units)')
PY
