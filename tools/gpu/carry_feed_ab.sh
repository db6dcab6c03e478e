# The device ingests of another commit's build (OLD=dir with its libhast.so and programs, built by hand, not committed) against this
# tree's, on one box, alternating, PAUSE s apart: every route that goes through carry_feed.h or the encoder slot of dz_device.h, and the
# host routes over the work area of ingest.h (BlockWork).
#   s00_fq / s00_fq_gz / s00_fa60   unshared_kmers --ingest device (hast_sq_feed; the inputs of tools/gpu/s00_ingest.sh and s00_ingest_fasta.sh)
#   s03_fq / s03_fq_bins_gz / s03_fa_bins_gz   classify_read --ingest device, without bins and with --bin-reads --gz-out (hast_rs; the
#                                   long reads of tools/gpu/classify_read_device.sh and classify_read_bins.sh)
#   route_gz                        classify --phase-reads --gz-out (hast_fq_set_route_gz; the sample of tools/gpu/route_gz.sh)
#   fake10x_feed                    fake_10x --convert device --inflate device (hast_tx_feed; the sample of tools/gpu/fake10x_feed.sh)
#   s03_fq_host                     classify_read --ingest host on the same long reads
#   s01_host_parse                  classify --host-parse on the routed-pairs sample
# LEGS="a b ..." runs only those legs (default: all of them).
# Per run: whole-process seconds, the phase's seconds as the program's --stats give them, the md5 of what it wrote (.gz files through
# gzip -dc).  Every run has its own time limit and the job ends at the first run that fails or whose products differ from the
# other build's.  At the end, per leg: both builds' means, OLD's spread (max - min) over its runs, and whether this tree's mean lies
# within OLD's mean + spread.
# usage (on a box with an MI355X, after the build): OLD=<dir> bash tools/gpu/carry_feed_ab.sh > profiles/carry_feed_ab.txt 2>&1
#   GENOME (default 20000000) COVERAGE (20) NLONG (5000) KEYS (2000000) NPAIRS (2000000) TXPAIRS (1000000) BARCODES (200000) RUNS (3) PAUSE (3)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
ROOT=$PWD
[ -n "$OLD" ] && [ -x $OLD/unshared_kmers ] || { echo "OLD=<dir of the other build> is needed"; exit 1; }
OLD=$(cd $OLD && pwd)
GENOME=${GENOME:-20000000}; COVERAGE=${COVERAGE:-20}; NLONG=${NLONG:-5000}; KEYS=${KEYS:-2000000}; NPAIRS=${NPAIRS:-2000000}; TXPAIRS=${TXPAIRS:-1000000}
BARCODES=${BARCODES:-200000}; RUNS=${RUNS:-3}; PAUSE=${PAUSE:-3}
LEGS=${LEGS:-s00_fq s00_fq_gz s00_fa60 s03_fq s03_fq_bins_gz s03_fa_bins_gz route_gz fake10x_feed s03_fq_host s01_host_parse}
wanted() { case " $LEGS " in *" $1 "*) return 0;; esac; return 1; }
D=$(mktemp -d /dev/shm/hast_cfab.XXXXXX) || exit 1
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free; OLD=$OLD"
# the inputs
mkdir -p $D/trio && tools/gen_trio $D/trio $GENOME $COVERAGE 150 1 16 || exit 1
for p in paternal maternal; do
  tools/pgzip1 $D/trio/${p}_0.fq $D/trio/${p}_0.fq.gz 6 16 || exit 1
  awk 'NR % 4 == 1 { print ">" substr($0, 2) } NR % 4 == 2 { for (i = 1; i <= length($0); i += 60) print substr($0, i, 60) }' $D/trio/${p}_0.fq > $D/trio/${p}_0.fa60 || exit 1
done
mkdir -p $D/long && tools/gen_fastq $D/long $NLONG $KEYS 1 31 20000 16 > /dev/null || exit 1
rm -f $D/long/r2.fq
awk 'NR%4==1{print ">" substr($0,2)} NR%4==2{print}' $D/long/r1.fq | fold -w 60 > $D/long/r1.fa || exit 1
mkdir -p $D/pairs && tools/gen_fastq $D/pairs $NPAIRS $KEYS $BARCODES 21 150 16 0 > /dev/null || exit 1
mkdir -p $D/tx
if wanted fake10x_feed; then
tools/gen_fastq $D/tx $TXPAIRS 1000 $BARCODES 21 150 16 0 > /dev/null || exit 1
gzip $D/tx/r1.fq & Z1=$!; gzip $D/tx/r2.fq & Z2=$!; wait $Z1 $Z2 || exit 1
fi
python3 - $BARCODES > $D/tx/map.txt <<'EOF'
import sys
for i in range(int(sys.argv[1])):
    if i % 10 == 9:
        continue
    name = "0_0_0" if i == 0 else "%d_%d_%d" % (i % 1536 + 1, (i // 1536) % 1536 + 1, i // (1536 * 1536) + 1)
    print(name + "\t" + "".join("ACGT"[(i * 2654435761 >> (2 * j)) & 3] for j in range(16)))
EOF
echo "== inputs: trio $GENOME x $COVERAGE ($(stat -c %s $D/trio/paternal_0.fq) bytes of .fq a parent), $NLONG long reads ($(stat -c %s $D/long/r1.fq) bytes of .fq), $NPAIRS pairs to route, $TXPAIRS pairs to convert"
# what a run left in its directory, names and plain bytes (stdout without the line that repeats the command; not classify's step_*_done,
# which hold the date)
products() { (cd $1 && for f in $(ls | grep -v '^err$\|^step_.*_done$' | sort); do echo "${f%.gz}"; case $f in *.gz) gzip -dc $f;; out.txt) grep -v '^CMD :' $f;; *) cat $f;; esac; done) | md5sum | cut -c1-16; }
# one run: $1 = leg, $2 = build (old / new), $3 = the sed expression that takes the phase's seconds out of err, the rest = the command
run() { local leg=$1 build=$2 phase=$3; shift 3
  local w=$D/w; rm -rf $w; mkdir -p $w
  local t0=$(now)
  (cd $w && timeout -k 10 200 "$@" > out.txt 2> err) || { echo "-- $leg $build FAILED rc=$?"; tail -5 $w/err; return 1; }
  local t1=$(now)
  MD5=$(products $w)
  echo "-- $leg $build: whole_s=$(python3 -c "print(round($t1-$t0,2))") phase_s=$(sed -n "$phase" $w/err | head -1) md5=$MD5"
  sleep $PAUSE; return 0; }
# one leg: $1 = name, $2 = program, $3 = phase expression, the rest = its arguments
leg() { local name=$1 exe=$2 phase=$3; shift 3
  wanted $name || return 0
  for i in $(seq 1 $RUNS); do
    run $name old "$phase" $OLD/$exe "$@" || exit 1; local m=$MD5
    run $name new "$phase" $ROOT/hast_amd/$exe "$@" || exit 1
    [ "$m" = "$MD5" ] || { echo "-- $name run $i: the products DIFFER"; exit 1; }
  done; }
S00='s/.*read+parse+count \([0-9.]*\) s.*/\1/p'
S03='s/.*read_phase=\([0-9.]*\).*/\1/p'
RGZ='s/.*lists_and_routing_s=\([0-9.]*\).*/\1/p'
S01='s/.* read_phase_s=\([0-9.]*\).*/\1/p'
T=$D/trio; L=$D/long; P=$D/pairs
{
leg s00_fq unshared_kmers "$S00" --paternal $T/paternal_0.fq --maternal $T/maternal_0.fq --thread 8 --table-gb 48 --stats --ingest device
leg s00_fq_gz unshared_kmers "$S00" --paternal $T/paternal_0.fq.gz --maternal $T/maternal_0.fq.gz --thread 8 --table-gb 48 --stats --ingest device
leg s00_fa60 unshared_kmers "$S00" --paternal $T/paternal_0.fa60 --maternal $T/maternal_0.fa60 --thread 8 --table-gb 48 --stats --ingest device --device-fasta
leg s03_fq classify_read "$S03" --hap $L/hap0.mer --hap $L/hap1.mer --read $L/r1.fq --format fastq --thread 16 --ingest device --stats
leg s03_fq_bins_gz classify_read "$S03" --hap $L/hap0.mer --hap $L/hap1.mer --read $L/r1.fq --format fastq --thread 16 --ingest device --stats --bin-reads --gz-out --bin-dir .
leg s03_fa_bins_gz classify_read "$S03" --hap $L/hap0.mer --hap $L/hap1.mer --read $L/r1.fa --format fasta --thread 16 --ingest device --stats --bin-reads --gz-out --bin-dir .
leg route_gz classify "$RGZ" --hap0 $P/hap0.mer --hap1 $P/hap1.mer --weight0 1.04 -t 16 --stats --phase-reads --read $P/r1.fq --read $P/r2.fq --gz-out
leg fake10x_feed fake_10x "$S03" $D/tx/r1.fq.gz $D/tx/r2.fq.gz $D/tx/map.txt --stats --convert device --inflate device
leg s03_fq_host classify_read "$S03" --hap $L/hap0.mer --hap $L/hap1.mer --read $L/r1.fq --format fastq --thread 16 --ingest host --stats
leg s01_host_parse classify "$S01" --hap0 $P/hap0.mer --hap1 $P/hap1.mer --weight0 1.04 -t 16 --stats --host-parse --read $P/r1.fq --read $P/r2.fq
} | tee $D/log.txt
[ ${PIPESTATUS[0]} -eq 0 ] || exit 1
python3 - $D/log.txt <<'EOF'
import re, sys
runs = {}
for line in open(sys.argv[1]):
    m = re.match(r"-- (\S+) (old|new): whole_s=(\S+) phase_s=(\S*) md5", line)
    if m:
        for what, x in (("whole", m.group(3)), ("phase", m.group(4))):
            if x:
                runs.setdefault((m.group(1), what), {}).setdefault(m.group(2), []).append(float(x))
print("== per leg: OLD's mean and spread (max - min), this tree's mean, and whether it lies within OLD's mean + spread")
for (leg, what), r in runs.items():
    old, new = r["old"], r["new"]
    mo, mn, spread = sum(old) / len(old), sum(new) / len(new), max(old) - min(old)
    print("%-16s %-5s old %.3f s (spread %.3f, runs %s)  new %.3f s (runs %s)  %s" % (leg, what, mo, spread, old, mn, new, "within" if mn <= mo + spread else "OUTSIDE"))
EOF
echo "== done"
