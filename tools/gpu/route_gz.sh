# classify --phase-reads --gz-out measured (DESIGN.md "Routed FASTQ deflated on the GPU"): ratio against zlib, lists + routing seconds
# with and without the flag, what the pipeline pays today behind the plain files (gzip -1 / -6 of one routed file), kernel times.
# Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.
# usage (on a box with an MI355X, after the build): bash tools/gpu/route_gz.sh > profiles/route_gz.txt 2>&1
#   NPAIRS (default 10000000 = 20M reads), KEYS (2000000 per haplotype), BARCODES (200000), PAIRS (4: alternating runs), STEPS (ratio time host prof)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NPAIRS=${NPAIRS:-10000000}; KEYS=${KEYS:-2000000}; BARCODES=${BARCODES:-200000}; PAIRS=${PAIRS:-4}
STEPS=${STEPS:-ratio time host prof}
has() { case " $STEPS " in *" $1 "*) return 0;; esac; return 1; }
D=$(mktemp -d /dev/shm/hast_rgz.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
PY=$PWD/hast_amd/classify
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free, / $(df -h /tmp | tail -1 | awk '{print $4}') free"
gen() {  # $1 = directory, $2 = GEN_FASTQ_QUAL
  mkdir -p $1 && GEN_FASTQ_QUAL=$2 tools/gen_fastq $1 $NPAIRS $KEYS $BARCODES 21 150 16 0 > /dev/null || return 1
  echo "== $1: $((2*NPAIRS)) reads of 150 bp, quality lines '${2:-constant}', $(stat -c %s $1/r1.fq) bytes per FASTQ file"; }
# one run: $1 = name, $2 = work directory's parent, rest = extra flags; prints the phase's seconds and the routed sizes
run() { local name=$1 base=$2; shift 2; local w=$base/w.$name; rm -rf $w; mkdir -p $w
  (cd $w && timeout -k 10 300 $PY --hap0 $IN/hap0.mer --hap1 $IN/hap1.mer --weight0 1.04 -t 16 --stats --phase-reads --read $IN/r1.fq --read $IN/r2.fq "$@" > out.tsv 2> err) || { echo "-- $name FAILED rc=$?"; tail -5 $w/err; return 1; }
  echo "-- $name: $(grep -h -o 'lists_and_routing_s=[0-9.]* lists_s=[0-9.]* routing_s=[0-9.]*' $w/err) $(grep -h -o 'waiting_for_gpu_s=[0-9.]* idle_s=[0-9.]*' $w/err) stdout md5=$(md5sum < $w/out.tsv | cut -c1-12) routed bytes on disk=$(cat $w/*.fastq $w/*.fastq.gz 2>/dev/null | wc -c)"
  grep -h "__stats_route_gz__" $w/err | sed 's/^/     /'; return 0; }

IN=$D/const
gen $D/const "" || exit 1
if has ratio; then
  gen $D/noisy noisy || exit 1
  for q in const noisy; do
    IN=$D/$q
    run ratio_$q $D --gz-out || exit 1
    w=$D/w.ratio_$q
    echo "   encoder on $q quality lines, per routed file (compressed / plain; zlib on the same plain bytes: 16-KB pieces at level 1 and 6, whole at 1 and 6; the leading members of a file, ~64 MB):"
    for f in $w/r1.fq.*.fastq.gz; do
      python3 tools/gpu/route_gz_ratio.py $f || exit 1
    done
    rm -rf $w
  done
  rm -rf $D/noisy
  IN=$D/const
fi
if has time; then
  echo "== lists + routing, alternating, 5 s between processes; outputs in /dev/shm"
  for i in $(seq 1 $PAIRS); do
    run plain_$i $D || exit 1; rm -rf $D/w.plain_$i; sleep 5
    run gz_$i $D --gz-out || exit 1; rm -rf $D/w.gz_$i; sleep 5
  done
  DISK=$(mktemp -d /tmp/hast_rgz.XXXXXX)
  echo "== the same once with the outputs on the box's disk ($DISK)"
  { run plain_disk $DISK && rm -rf $DISK/w.plain_disk && sleep 5 && run gz_disk $DISK --gz-out; } || { rm -rf $DISK; exit 1; }
  rm -rf $DISK
fi
if has host; then
  echo "== what the pipeline pays behind the plain files today: gzip of ONE routed file on one host thread"
  run keep $D || exit 1
  f=$(ls -S $D/w.keep/*.fastq | head -1)
  for lv in 1 6; do t0=$(now); gzip -$lv -c $f > $D/one.gz; t1=$(now); echo "-- gzip -$lv $(basename $f): $(stat -c %s $f) -> $(stat -c %s $D/one.gz) bytes in $(el $t0 $t1) s"; done
  rm -rf $D/w.keep $D/one.gz
fi
if has prof; then
  echo "== kernel times of one --gz-out run (rocprofv3 --kernel-trace --stats, a run of its own, no counters)"
  mkdir -p $D/prof && (cd $D/prof && timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $D/prof/out -o rgz -- $PY --hap0 $IN/hap0.mer --hap1 $IN/hap1.mer --weight0 1.04 -t 16 --phase-reads --gz-out --read $IN/r1.fq --read $IN/r2.fq > out.tsv 2> err) || { echo "-- profile run FAILED rc=$?"; tail -5 $D/prof/err; exit 1; }
  python3 - $(find $D/prof/out -name '*kernel_stats.csv' | head -1) <<'EOF'
import csv, sys
for i, r in enumerate(csv.DictReader(open(sys.argv[1]))):
    if i < 12:
        print("   %-28s calls=%-6s total_ms=%-10.2f avg_us=%-10.1f %s%%" % (r["Name"].split("(")[0][-28:], r["Calls"], int(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e3, r["Percentage"]))
EOF
fi
echo "== done"
