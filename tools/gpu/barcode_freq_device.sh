# barcode_freq --count device measured against --count host: whole-process seconds of both routes on the same
# read-1 file, as .gz and plain, alternating; the [stats] lines of every run; whether both routes print the same rows; and, in a run
# of its own, the kernel times of one device run under rocprofv3 --kernel-trace --stats.
# The sample is section 11's read-1 file: 1M reads of tools/gen_fastq (150 bp) over 200 000 barcodes, in /dev/shm.
# Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.
# usage (on a box with an MI355X, after the build and `make -C tools gen_fastq`): bash tools/gpu/barcode_freq_device.sh > profiles/barcode_freq.txt 2>&1
#   NREADS (default 1000000), BARCODES (200000), PAIRS (3: alternating runs host / device per input), PROFILE (1: the rocprofv3 run)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NREADS=${NREADS:-1000000}; BARCODES=${BARCODES:-200000}; PAIRS=${PAIRS:-3}; PROFILE=${PROFILE:-1}
D=$(mktemp -d /dev/shm/hast_bf.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
EXE=$PWD/hast_amd/barcode_freq
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free"
mkdir -p $D/in && tools/gen_fastq $D/in $NREADS 1000 $BARCODES 21 150 16 0 > /dev/null || exit 1
rm -f $D/in/hap0.mer $D/in/hap1.mer $D/in/r2.fq
gzip -k $D/in/r1.fq || exit 1
echo "== sample: $NREADS reads of 150 bp, $(stat -c %s $D/in/r1.fq) bytes of .fq, $(stat -c %s $D/in/r1.fq.gz) bytes of .fq.gz"
# one run: $1 = name, $2 = input, rest = flags; prints the whole-process seconds, the stats lines and the md5 of the rows
run() { local name=$1 in=$2; shift 2
  local t0=$(now)
  timeout -k 10 240 $EXE --stats "$@" $in > $D/out.$name 2> $D/err.$name || { echo "-- $name FAILED rc=$?"; tail -5 $D/err.$name; return 1; }
  local t1=$(now)
  MD5=$(md5sum < $D/out.$name | cut -c1-32)
  echo "-- $name: whole process $(el $t0 $t1) s; $(wc -l < $D/out.$name) rows, md5 $MD5"
  grep -h "^\[stats\]" $D/err.$name | sed 's/^/     /'
  SECONDS_OF=$(el $t0 $t1); rm -f $D/out.$name $D/err.$name; return 0; }
WON=0; ALL=0
for kind in gz plain; do
  IN=$D/in/r1.fq; [ $kind = gz ] && IN=$D/in/r1.fq.gz
  echo "== $kind input: host route (--count host) and device route (--count device, the default), alternating, 5 s between processes"
  for i in $(seq 1 $PAIRS); do
    run host_${kind}_$i $IN --count host || exit 1; H=$SECONDS_OF; HMD5=$MD5; sleep 5
    run device_${kind}_$i $IN --count device || exit 1; G=$SECONDS_OF; sleep 5
    [ "$MD5" = "$HMD5" ] || { echo "-- $kind pair $i: the rows DIFFER"; exit 1; }
    ALL=$((ALL+1)); python3 -c "import sys; sys.exit(0 if $G < $H else 1)" && WON=$((WON+1))
    echo "-- $kind pair $i: host $H s, device $G s, rows identical"
  done
done
echo "== the device route took less whole-process time than the host route in $WON of $ALL pairs"
if [ "$PROFILE" = 1 ]; then
  echo "== kernel times of one device run on the .gz input (rocprofv3 --kernel-trace --stats, a run of its own)"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D/prof -o bf -- $EXE $D/in/r1.fq.gz > /dev/null 2> $D/err.prof || { echo "-- the profiled run FAILED rc=$?"; tail -5 $D/err.prof; exit 1; }
  ST=$(find $D/prof -name '*kernel_stats.csv' | head -1)
  [ -n "$ST" ] || { echo "-- no kernel_stats.csv under $D/prof:"; find $D/prof -type f | head; exit 1; }
  head -1 $ST; grep -E 'k_fq_field2|k_tally_add|k_fq_name_claim|k_fq_records|k_fq_index|k_fq_count|k_fq_scan|k_fq_begin' $ST
fi
echo "== done"
