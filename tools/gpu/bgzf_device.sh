# classify --bgzf device measured against its two yardsticks: the same generated reads as blocked gzip (BGZF,
# tools/to_bgzf) and as ordinary gzip (gzip -6), through `classify --stats` three ways, RUNS runs each, the legs alternating:
#   bgzf_host     BGZF on the host route (the default: bgzf_reader.h on host threads, the inflated bytes cross PCIe)
#   bgzf_device   BGZF with --bgzf device (hast_gz_open_blocked: a wave per member, bz_kernels.hip)
#   gz_device     the ordinary .gz on the device route (hast_gz_open: search, chain, windows, translate)
# The three stdouts must be md5-equal.  Medians and ranges of read_phase_s and of the __stats_bgzf__ seconds are printed at the end.
# Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.  PAUSE
# seconds lie between two processes.
# usage (on a box with an MI355X, after the build and `make -C tools gen_fastq to_bgzf`): bash tools/gpu/bgzf_device.sh > profiles/bgzf_device.txt 2>&1
#   NPAIRS (default 10000000: 20M reads in two files), KEYS (5000000), BARCODES (100000), RUNS (5), THREADS (16), PAUSE (3)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NPAIRS=${NPAIRS:-10000000}; KEYS=${KEYS:-5000000}; BARCODES=${BARCODES:-100000}; RUNS=${RUNS:-5}; THREADS=${THREADS:-16}; PAUSE=${PAUSE:-3}
D=$(mktemp -d /dev/shm/hast_bz.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
EXE=$PWD/hast_amd/classify
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free"
tools/gen_fastq $D $NPAIRS $KEYS $BARCODES 21 150 $THREADS 0 > /dev/null || exit 1
T0=$(now)
for r in r1 r2; do
  tools/to_bgzf $D/$r.fq $D/$r.bgzf.fq.gz $THREADS 6 || exit 1
done
T1=$(now)
(gzip -6 -c $D/r1.fq > $D/r1.plain.fq.gz & gzip -6 -c $D/r2.fq > $D/r2.plain.fq.gz & wait) || exit 1
echo "== $((2 * NPAIRS)) reads of 150 bp: $(stat -c %s $D/r1.fq) + $(stat -c %s $D/r2.fq) bytes of FASTQ; BGZF $(stat -c %s $D/r1.bgzf.fq.gz) + $(stat -c %s $D/r2.bgzf.fq.gz) (to_bgzf, level 6, $(el $T0 $T1) s); gzip -6 $(stat -c %s $D/r1.plain.fq.gz) + $(stat -c %s $D/r2.plain.fq.gz)"
rm -f $D/r1.fq $D/r2.fq
ARGS="--hap0 $D/hap0.mer --hap1 $D/hap1.mer --weight0 1.04 --thread $THREADS --stats"
# one run: $1 = leg, $2 = run number, the rest = the inputs and flags of the leg
run() { local leg=$1 i=$2; shift 2
  local t0=$(now)
  timeout -k 10 300 $EXE $ARGS "$@" > $D/out 2> $D/err || { echo "-- $leg run $i FAILED rc=$?"; tail -5 $D/err; return 1; }
  local t1=$(now)
  MD5=$(md5sum < $D/out | cut -c1-32)
  local phase=$(grep -o 'read_phase_s=[0-9.]*' $D/err | cut -d= -f2)
  echo "-- $leg run $i: whole process $(el $t0 $t1) s, read_phase_s $phase; $(wc -l < $D/out) rows, md5 $MD5"
  grep -h "^__stats_bgzf__\|^__stats_gz__\|^__stats_read_phase__" $D/err | sed 's/^/     /'
  echo "$leg read_phase_s $phase" >> $D/figures
  grep -h "^__stats_bgzf__" $D/err | tr ' ' '\n' | grep -E '^(read_s|upload_s|kernels_s|producer_waited_for_reader_s)=' | sed "s/^/$leg /; s/=/ /" >> $D/figures
  rm -f $D/out $D/err; return 0; }
for i in $(seq 1 $RUNS); do
  run bgzf_host $i --read $D/r1.bgzf.fq.gz --read $D/r2.bgzf.fq.gz || exit 1; H=$MD5; sleep $PAUSE
  run bgzf_device $i --read $D/r1.bgzf.fq.gz --read $D/r2.bgzf.fq.gz --bgzf device || exit 1; B=$MD5; sleep $PAUSE
  run gz_device $i --read $D/r1.plain.fq.gz --read $D/r2.plain.fq.gz || exit 1; G=$MD5; sleep $PAUSE
  [ "$H" = "$B" ] && [ "$H" = "$G" ] || { echo "-- run $i: the three stdouts DIFFER ($H $B $G)"; exit 1; }
  echo "-- run $i: the three stdouts are md5-equal"
done
echo "== medians and ranges over $RUNS runs (seconds; the __stats_bgzf__ figures are per input file, two a run)"
python3 - $D/figures <<'EOF'
import statistics, sys
fig = {}
for line in open(sys.argv[1]):
    leg, name, v = line.split()
    fig.setdefault((leg, name), []).append(float(v))
for (leg, name), v in sorted(fig.items()):
    print("%-12s %-30s median %.3f  range %.3f .. %.3f  (n = %d)" % (leg, name, statistics.median(v), min(v), max(v), len(v)))
EOF
echo "== done"
