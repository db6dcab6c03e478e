# classify_read --ingest device measured against --ingest host: whole-process seconds and the read phase of
# both routes on the same generated files, alternating, RUNS runs per leg; the [stats] lines of every run; whether both routes print
# the same rows.  The inputs, in /dev/shm:
#   long reads  NLONG x 20-kb reads of tools/gen_fastq (K = 31, KEYS keys per haplotype: tests/e2e/cli_e2e_s03.sh's generator) as
#               FASTQ, as .fq.gz and as 60-column FASTA
#   short reads NSHORT x 1-kb reads as 60-column FASTA (NSHORT=0 leaves the leg out)
# Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.  A few seconds
# lie between two processes.
# usage (on a box with an MI355X, after the build and `make -C tools gen_fastq`): bash tools/gpu/classify_read_device.sh > profiles/classify_read_ingest.txt 2>&1
#   NLONG (default 15000), NSHORT (2000000), KEYS (2000000), RUNS (3), THREADS (16), PAUSE (4)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NLONG=${NLONG:-15000}; NSHORT=${NSHORT:-2000000}; KEYS=${KEYS:-2000000}; RUNS=${RUNS:-3}; THREADS=${THREADS:-16}; PAUSE=${PAUSE:-4}
D=$(mktemp -d /dev/shm/hast_rs.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
EXE=$PWD/hast_amd/classify_read
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free"
to_fasta() { awk 'NR%4==1{print ">" substr($0,2)} NR%4==2{print}' $1 | fold -w 60 > $2; }
mkdir -p $D/long && tools/gen_fastq $D/long $NLONG $KEYS 1 31 20000 16 > /dev/null || exit 1
rm -f $D/long/r2.fq
gzip -1 -k $D/long/r1.fq && to_fasta $D/long/r1.fq $D/long/r1.fa || exit 1
echo "== long reads: $NLONG x 20 kb, $(stat -c %s $D/long/r1.fq) bytes of .fq, $(stat -c %s $D/long/r1.fq.gz) of .fq.gz, $(stat -c %s $D/long/r1.fa) of 60-column .fa; $KEYS 31-mers per haplotype"
if [ "$NSHORT" -gt 0 ]; then
  mkdir -p $D/short && tools/gen_fastq $D/short $((NSHORT / 2)) 1000 1 31 1000 16 > /dev/null || exit 1      # (pairs: both files' reads are used)
  cat $D/short/r2.fq >> $D/short/r1.fq && rm -f $D/short/r2.fq && to_fasta $D/short/r1.fq $D/short/r1.fa && rm -f $D/short/r1.fq $D/short/hap0.mer $D/short/hap1.mer || exit 1
  echo "== short reads: $NSHORT x 1 kb, $(stat -c %s $D/short/r1.fa) bytes of 60-column .fa"
fi
# one run: $1 = name, $2 = input, $3 = format, $4 = route; prints the whole-process seconds, the stats lines and the md5 of the rows
run() { local name=$1 in=$2 fmt=$3 route=$4
  local t0=$(now)
  timeout -k 10 300 $EXE --hap $D/long/hap0.mer --hap $D/long/hap1.mer --read $in --format $fmt --thread $THREADS --ingest $route --stats > $D/out.$name 2> $D/err.$name \
    || { echo "-- $name FAILED rc=$?"; tail -5 $D/err.$name; return 1; }
  local t1=$(now)
  MD5=$(md5sum < $D/out.$name | cut -c1-32)
  PHASE=$(grep -o 'read_phase=[0-9.]*' $D/err.$name | cut -d= -f2)
  echo "-- $name: whole process $(el $t0 $t1) s, read phase $PHASE s; $(wc -l < $D/out.$name) rows, md5 $MD5"
  grep -h "^\[stats\]" $D/err.$name | sed 's/^/     /'
  grep -h "WARN" $D/err.$name | sed 's/^/     /'
  SECONDS_OF=$(el $t0 $t1); rm -f $D/out.$name $D/err.$name; return 0; }
leg() { local kind=$1 in=$2 fmt=$3
  echo "== $kind: host route (--ingest host, the default) and device route (--ingest device), alternating, $PAUSE s between processes"
  for i in $(seq 1 $RUNS); do
    run host_${kind}_$i $in $fmt host || exit 1; H=$SECONDS_OF; HP=$PHASE; HMD5=$MD5; sleep $PAUSE
    run device_${kind}_$i $in $fmt device || exit 1; G=$SECONDS_OF; GP=$PHASE; sleep $PAUSE
    [ "$MD5" = "$HMD5" ] || { echo "-- $kind run $i: the rows DIFFER"; exit 1; }
    echo "-- $kind run $i: whole process host $H s, device $G s; read phase host $HP s, device $GP s; rows identical"
  done; }
leg long_fastq $D/long/r1.fq fastq
leg long_fastq_gz $D/long/r1.fq.gz fastq
leg long_fasta $D/long/r1.fa fasta
[ "$NSHORT" -gt 0 ] && leg short_fasta $D/short/r1.fa fasta
echo "== done"
