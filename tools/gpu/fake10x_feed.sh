# fake_10x --convert device --inflate device (the paired feed: inputs inflated on the GPU, deflate beside the next step) measured against
# --convert device as it was (inputs inflated on the host, every step synchronous): whole-process seconds of both
# routes on the same files, alternating, the [stats] lines of every run, and whether both routes' outputs decode to the same bytes.
# The sample is section 11's: 1M pairs of tools/gen_fastq (150 bp, gzip'ed) and a map that keeps 90 % of 200 000 barcodes.
# Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.  No profiler.
# usage (on a box with an MI355X, after the build): bash tools/gpu/fake10x_feed.sh > profiles/fake10x_feed.txt 2>&1
#   NPAIRS (default 1000000), BARCODES (200000), PAIRS (3: alternating runs --convert device / --convert device --inflate device)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NPAIRS=${NPAIRS:-1000000}; BARCODES=${BARCODES:-200000}; PAIRS=${PAIRS:-3}
D=$(mktemp -d /dev/shm/hast_f10xfeed.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
EXE=$PWD/hast_amd/fake_10x
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free"
mkdir -p $D/in && tools/gen_fastq $D/in $NPAIRS 1000 $BARCODES 21 150 16 0 > /dev/null || exit 1
rm -f $D/in/hap0.mer $D/in/hap1.mer
gzip $D/in/r1.fq & Z1=$!; gzip $D/in/r2.fq & Z2=$!; wait $Z1 $Z2 || exit 1
# the map: barcode id -> a 16-base 10x barcode, every tenth barcode left out (gen_fastq's names: 0_0_0, else a_b_c)
python3 - $BARCODES > $D/in/map.txt <<'EOF'
import sys
for i in range(int(sys.argv[1])):
    if i % 10 == 9:
        continue
    name = "0_0_0" if i == 0 else "%d_%d_%d" % (i % 1536 + 1, (i // 1536) % 1536 + 1, i // (1536 * 1536) + 1)
    print(name + "\t" + "".join("ACGT"[(i * 2654435761 >> (2 * j)) & 3] for j in range(16)))
EOF
echo "== sample: $NPAIRS pairs of 150 bp, $(stat -c %s $D/in/r1.fq.gz) + $(stat -c %s $D/in/r2.fq.gz) bytes of .fq.gz, $(wc -l < $D/in/map.txt) of $BARCODES barcodes in the map"
# one run: $1 = name, rest = flags; prints the whole-process seconds, the stats lines and the md5 of both decoded outputs
run() { local name=$1; shift; local w=$D/w.$name; rm -rf $w; mkdir -p $w
  local t0=$(now)
  (cd $w && timeout -k 10 240 $EXE $D/in/r1.fq.gz $D/in/r2.fq.gz $D/in/map.txt --stats "$@" > out.txt 2> err) || { echo "-- $name FAILED rc=$?"; tail -5 $w/err; return 1; }
  local t1=$(now)
  echo "-- $name: whole process $(el $t0 $t1) s; $(tail -1 $w/out.txt)"
  grep -h "^\[stats\]" $w/err | sed 's/^/     /'
  MD5=$(for s in 1 2; do gzip -dc $w/SampleName_S1_L001_R${s}_001.fastq.gz | md5sum | cut -c1-32; done | tr '\n' ' ')
  echo "     decoded outputs md5: $MD5; bytes on disk $(cat $w/*.fastq.gz | wc -c)"
  SECONDS_OF=$(el $t0 $t1); rm -rf $w; return 0; }
echo "== staged route (--convert device) and feed route (--convert device --inflate device), alternating, 5 s between processes"
WON=0
for i in $(seq 1 $PAIRS); do
  run staged_$i --convert device || exit 1; H=$SECONDS_OF; HMD5=$MD5; sleep 5
  run feed_$i --convert device --inflate device || exit 1; G=$SECONDS_OF; sleep 5
  [ "$MD5" = "$HMD5" ] || { echo "-- pair $i: the outputs DIFFER"; exit 1; }
  python3 -c "import sys; sys.exit(0 if $G < $H else 1)" && WON=$((WON+1))
  echo "-- pair $i: staged $H s, feed $G s, outputs identical after gzip -dc"
done
echo "== the feed route took less whole-process time than the staged route in $WON of $PAIRS pairs"
echo "== done"
