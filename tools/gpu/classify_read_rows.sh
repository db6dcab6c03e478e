# classify_read --rows device measured against its yardsticks: who formats the rows of the device ingest.  Two
# inputs on /dev/shm, both from tools/gen_fastq: short reads (NSHORT records of 150 bp, FASTQ: about 190 000 rows per 64-MB block) and
# long reads (NLONG records of 20 kb as 60-column FASTA: about 3 000 rows per block).  Per input three legs, all with
# --ingest device --stats, RUNS runs each, the legs alternating, PAUSE seconds between two processes:
#   parent   the parent commit's build ($PARENT: that commit's classify_read + libhast.so, built by hand, not committed)
#   host     this tree with --rows host
#   device   this tree with --rows device
# Per run: read_phase and rows of `[stats] seconds:` (rows = host seconds spent on rows), the `[stats] rows:` line, the md5 of stdout.
# Asserted: the three stdouts are md5-equal in every round and the device leg made its rows on the device (views_on_host=0,
# fallback=none).  Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.
# usage (on a box with an MI355X, after the build and `make -C tools gen_fastq`):
#   PARENT=dir bash tools/gpu/classify_read_rows.sh > profiles/classify_read_rows.txt 2>&1
#   NSHORT (default 4000000), NLONG (15000), KEYS (2000000), RUNS (5), THREADS (16), PAUSE (3)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NSHORT=${NSHORT:-4000000}; NLONG=${NLONG:-15000}; KEYS=${KEYS:-2000000}; RUNS=${RUNS:-5}; THREADS=${THREADS:-16}; PAUSE=${PAUSE:-3}
PARENT=$(cd "${PARENT:-tools/ab_old}" 2>/dev/null && pwd)
[ -n "$PARENT" ] && [ -x $PARENT/classify_read ] && [ -f $PARENT/libhast.so ] || { echo "PARENT: a directory with the parent commit's classify_read and libhast.so"; exit 1; }
D=$(mktemp -d /dev/shm/hast_rr.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
NEW=$PWD/hast_amd/classify_read
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free"
mkdir -p $D/long $D/short
tools/gen_fastq $D/long $NLONG $KEYS 1 31 20000 16 > /dev/null || exit 1
rm -f $D/long/r2.fq
awk 'NR%4==1{print ">" substr($0,2)} NR%4==2{print}' $D/long/r1.fq | fold -w 60 > $D/long/r1.fa && rm -f $D/long/r1.fq || exit 1
tools/gen_fastq $D/short $((NSHORT / 2)) 1000 1 31 150 16 > /dev/null || exit 1           # (pairs: both files' reads are used)
cat $D/short/r2.fq >> $D/short/r1.fq && rm -f $D/short/r2.fq $D/short/hap0.mer $D/short/hap1.mer || exit 1
echo "== short reads: $NSHORT x 150 bp, $(stat -c %s $D/short/r1.fq) bytes of .fq; long reads: $NLONG x 20 kb, $(stat -c %s $D/long/r1.fa) bytes of 60-column .fa; $KEYS 31-mers per haplotype"
cat $D/short/r1.fq $D/long/r1.fa > /dev/null
# one run: $1 = leg, $2 = input's name, $3 = run number, $4 = the program, the rest = the leg's flags
run() { local leg=$1 kind=$2 i=$3 exe=$4; shift 4
  timeout -k 10 300 $exe --hap $D/long/hap0.mer --hap $D/long/hap1.mer $ARGS --thread $THREADS --ingest device --stats "$@" > $D/out.$leg 2> $D/err.$leg \
    || { echo "-- $kind $leg run $i FAILED rc=$?"; tail -5 $D/err.$leg; return 1; }
  MD5=$(md5sum < $D/out.$leg | cut -c1-32)
  local phase=$(grep -o 'read_phase=[0-9.]*' $D/err.$leg | cut -d= -f2) rows=$(grep -o ' rows=[0-9.]*' $D/err.$leg | cut -d= -f2)
  echo "-- $kind $leg run $i: read_phase $phase s, rows $rows s; $(wc -l < $D/out.$leg) rows, $(stat -c %s $D/out.$leg) bytes, stdout md5 $MD5"
  grep -h "^\[stats\]" $D/err.$leg | sed 's/^/     /'
  grep -h "WARN" $D/err.$leg | sed 's/^/     /'
  if [ $leg = device ]; then grep -q "^\[stats\] rows: route=device views_on_device=[0-9]* views_on_host=0 .*fallback=none" $D/err.$leg || { echo "-- the device leg did not make its rows on the device"; return 1; }; fi
  echo "$kind $leg read_phase $phase" >> $D/figures
  echo "$kind $leg rows $rows" >> $D/figures
  rm -f $D/out.$leg $D/err.$leg
  return 0; }
for kind in short long; do
  [ $kind = short ] && ARGS="--read $D/short/r1.fq --format fastq" || ARGS="--read $D/long/r1.fa --format fasta"
  echo "== $kind reads: parent, --rows host, --rows device, alternating, $RUNS runs each, $PAUSE s between processes"
  for i in $(seq 1 $RUNS); do
    run parent $kind $i $PARENT/classify_read || exit 1; P=$MD5; sleep $PAUSE
    run host $kind $i $NEW --rows host || exit 1; H=$MD5; sleep $PAUSE
    run device $kind $i $NEW --rows device || exit 1; V=$MD5; sleep $PAUSE
    [ "$P" = "$H" ] && [ "$P" = "$V" ] || { echo "-- $kind run $i: the three stdouts DIFFER ($P $H $V)"; exit 1; }
    echo "-- $kind run $i: the three stdouts are md5-equal"
  done
done
echo "== medians and ranges over $RUNS runs (seconds; rows = host seconds spent on rows)"
python3 - $D/figures <<'EOF'
import statistics, sys
fig = {}
for line in open(sys.argv[1]):
    kind, leg, name, v = line.split()
    fig.setdefault((kind, name, leg), []).append(float(v))
for (kind, name, leg), v in sorted(fig.items()):
    print("%-6s %-11s %-7s median %.3f  range %.3f .. %.3f  (n = %d)  %s" % (kind, name, leg, statistics.median(v), min(v), max(v), len(v), " ".join("%.3f" % x for x in v)))
EOF
echo "== done"
