# classify_read --bin-reads measured: what routing the reads to haplotype files costs the device route, and how
# the device route compares with the host route doing the same.  On the four inputs of tools/gpu/classify_read_device.sh, per input
# and RUNS times, alternating:
#   device            --ingest device, no bins (and, with PARENT set, the same run of the parent commit's build: PARENT/classify_read)
#   device+bins       --ingest device --bin-reads             host+bins      --ingest host --bin-reads
#   device+bins+gz    --ingest device --bin-reads --gz-out    host+bins+gz   --ingest host --bin-reads --gz-out
# Whole-process seconds, the read phase, the [stats] lines; whether all legs print the same rows and both routes leave the same bytes
# (the .gz files through gzip -dc).  The bins go to /dev/shm, as the inputs come from there.
# Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.  A few seconds
# lie between two processes.
# usage (on a box with an MI355X, after the build and `make -C tools gen_fastq`): bash tools/gpu/classify_read_bins.sh > profiles/classify_read_bins.txt 2>&1
#   NLONG (default 15000), NSHORT (2000000), KEYS (2000000), RUNS (3), THREADS (16), PAUSE (4), PARENT (unset)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NLONG=${NLONG:-15000}; NSHORT=${NSHORT:-2000000}; KEYS=${KEYS:-2000000}; RUNS=${RUNS:-3}; THREADS=${THREADS:-16}; PAUSE=${PAUSE:-4}
D=$(mktemp -d /dev/shm/hast_rb.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
EXE=$PWD/hast_amd/classify_read
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free"
[ -n "$PARENT" ] && echo "== parent build: $PARENT/classify_read"
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
# one run: $1 = name, $2 = input, $3 = format, $4 = program, $5 = route, the rest = further flags; prints the whole-process seconds, the
# stats lines, the md5 of the rows and, with bins, the md5 of the three files' plain bytes
run() { local name=$1 in=$2 fmt=$3 exe=$4 route=$5; shift 5
  local bins=""; case " $* " in *" --bin-reads "*) mkdir -p $D/bins.$name; bins="--bin-dir $D/bins.$name";; esac
  local t0=$(now)
  timeout -k 10 300 $exe --hap $D/long/hap0.mer --hap $D/long/hap1.mer --read $in --format $fmt --thread $THREADS --ingest $route --stats "$@" $bins > $D/out.$name 2> $D/err.$name \
    || { echo "-- $name FAILED rc=$?"; tail -5 $D/err.$name; return 1; }
  local t1=$(now)
  MD5=$(md5sum < $D/out.$name | cut -c1-32)
  PHASE=$(grep -o 'read_phase=[0-9.]*' $D/err.$name | cut -d= -f2)
  BMD5=none
  if [ -n "$bins" ]; then
    BMD5=$(for f in $(ls $D/bins.$name | sort); do echo "${f%.gz}"; case $f in *.gz) gzip -dc $D/bins.$name/$f;; *) cat $D/bins.$name/$f;; esac; done | md5sum | cut -c1-32)
    echo "-- $name: whole process $(el $t0 $t1) s, read phase $PHASE s; $(wc -l < $D/out.$name) rows, md5 $MD5; $(du -sb $D/bins.$name | cut -f1) bytes of bins, plain md5 $BMD5"
    rm -rf $D/bins.$name
  else
    echo "-- $name: whole process $(el $t0 $t1) s, read phase $PHASE s; $(wc -l < $D/out.$name) rows, md5 $MD5"
  fi
  grep -h "^\[stats\]" $D/err.$name | sed 's/^/     /'
  grep -h "WARN" $D/err.$name | sed 's/^/     /'
  SECONDS_OF=$(el $t0 $t1); rm -f $D/out.$name $D/err.$name; return 0; }
leg() { local kind=$1 in=$2 fmt=$3
  echo "== $kind: the device route without bins, then both routes with --bin-reads, plain and --gz-out, alternating, $PAUSE s between processes"
  for i in $(seq 1 $RUNS); do
    local line="-- $kind run $i: whole process / read phase:"
    if [ -n "$PARENT" ]; then
      run parent_device_${kind}_$i $in $fmt $PARENT/classify_read device || exit 1; line="$line parent's device $SECONDS_OF / $PHASE s,"; sleep $PAUSE
    fi
    run device_${kind}_$i $in $fmt $EXE device && { line="$line device $SECONDS_OF / $PHASE s,"; ROWS=$MD5; sleep $PAUSE; } &&
      run device_bins_${kind}_$i $in $fmt $EXE device --bin-reads && { line="$line device+bins $SECONDS_OF / $PHASE s,"; DB=$BMD5; R1=$MD5; sleep $PAUSE; } &&
      run host_bins_${kind}_$i $in $fmt $EXE host --bin-reads && { line="$line host+bins $SECONDS_OF / $PHASE s,"; HB5=$BMD5; R2=$MD5; sleep $PAUSE; } &&
      run device_bins_gz_${kind}_$i $in $fmt $EXE device --bin-reads --gz-out && { line="$line device+bins+gz $SECONDS_OF / $PHASE s,"; DZ=$BMD5; R3=$MD5; sleep $PAUSE; } &&
      run host_bins_gz_${kind}_$i $in $fmt $EXE host --bin-reads --gz-out && { line="$line host+bins+gz $SECONDS_OF / $PHASE s"; HZ=$BMD5; R4=$MD5; sleep $PAUSE; } || exit 1
    [ "$ROWS" = "$R1" ] && [ "$ROWS" = "$R2" ] && [ "$ROWS" = "$R3" ] && [ "$ROWS" = "$R4" ] || { echo "-- $kind run $i: the rows DIFFER"; exit 1; }
    [ "$DB" = "$HB5" ] && [ "$DB" = "$DZ" ] && [ "$DB" = "$HZ" ] || { echo "-- $kind run $i: the bins DIFFER"; exit 1; }
    echo "$line; rows and bins identical"
  done; }
leg long_fastq $D/long/r1.fq fastq
leg long_fastq_gz $D/long/r1.fq.gz fastq
leg long_fasta $D/long/r1.fa fasta
[ "$NSHORT" -gt 0 ] && leg short_fasta $D/short/r1.fa fasta
echo "== done"
