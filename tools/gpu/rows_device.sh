# classify --rows device measured against its yardsticks: the inputs of profiles/round6_cli_cardinality.txt (10M read
# pairs of 150 bp over 1M and over 10M barcodes, 5M + 5M 21-mers, tools/gen_fastq), the output table made three ways, RUNS runs each, the
# legs alternating, PAUSE seconds between two processes:
#   parent   the parent commit's binaries ($PARENT: that commit's classify + libhast.so, built by hand, not committed)
#   host     this tree with --rows host
#   device   this tree with --rows device
# once without and once with --phase-reads.  Per run: counters_back_s + sort_print_s of __stats_phases__ (with --phase-reads sort_print_s
# holds the lists and the routing: lists_s and routing_s of __stats_phase_reads__ are shown beside it) and, on the device leg, the steps of
# __stats_rows__.  Asserted: the three stdouts are md5-equal in every round, the device leg took the device route, and with --phase-reads
# the three lists and filter_reads.log of the legs are the same bytes.
# Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.
# usage (on a box with an MI355X, after the build and `make -C tools gen_fastq`):
#   PARENT=dir bash tools/gpu/rows_device.sh > profiles/rows_device.txt 2>&1
#   BARCODES (default "1000000 10000000"), NPAIRS (10000000), KEYS (5000000), RUNS (3), THREADS (32), PAUSE (3), MODES ("plain phase")
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
unset HAST_ROWS
BARCODES=${BARCODES:-1000000 10000000}; NPAIRS=${NPAIRS:-10000000}; KEYS=${KEYS:-5000000}; RUNS=${RUNS:-3}; THREADS=${THREADS:-32}; PAUSE=${PAUSE:-3}
MODES=${MODES:-plain phase}
PARENT=$(cd "${PARENT:-tools/ab_old}" 2>/dev/null && pwd)
[ -n "$PARENT" ] && [ -x $PARENT/classify ] && [ -f $PARENT/libhast.so ] || { echo "PARENT: a directory with the parent commit's classify and libhast.so"; exit 1; }
D=$(mktemp -d /dev/shm/hast_rows.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
NEW=$PWD/hast_amd/classify
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free"
# one run: $1 = leg, $2 = mode, $3 = run number, $4 = the program, the rest = the leg's flags; its files stay in $D/w.$leg until the leg's next run
run() { local leg=$1 mode=$2 i=$3 exe=$4; shift 4
  local w=$D/w.$leg; rm -rf $w; mkdir -p $w
  local t0=$(now)
  (cd $w && timeout -k 10 300 $exe $ARGS "$@" > out.tsv 2> err) || { echo "-- $leg $mode run $i FAILED rc=$?"; tail -5 $w/err; return 1; }
  local t1=$(now)
  MD5=$(md5sum < $w/out.tsv | cut -c1-32)
  local back=$(grep -h -o ' counters_back_s=[0-9.]*' $w/err | cut -d= -f2) print=$(grep -h -o ' sort_print_s=[0-9.]*' $w/err | cut -d= -f2)
  echo "-- $leg $mode run $i: whole process $(el $t0 $t1) s, counters_back_s $back + sort_print_s $print = $(python3 -c "print(round($back+$print,3))"); rows $(wc -l < $w/out.tsv); stdout md5 $MD5"
  grep -h -o 'lists_and_routing_s=[0-9.]* lists_s=[0-9.]* routing_s=[0-9.]* route=[a-z]*' $w/err | sed 's/^/     /'
  grep -h "^__stats_rows__" $w/err | sed 's/^/     /'
  if [ $leg = device ]; then grep -q "^__stats_rows__ route=device fallback=none" $w/err || { echo "-- the device leg did not take the device route"; return 1; }; fi
  echo "$leg ${mode}_table_s $(python3 -c "print($back+$print)")" >> $D/figures.$NBC
  [ $mode = phase ] && echo "$leg phase_lists_s $(grep -h -o ' lists_s=[0-9.]*' $w/err | cut -d= -f2)" >> $D/figures.$NBC
  return 0; }
for NBC in $BARCODES; do
  echo "== $NBC barcodes, $NPAIRS read pairs of 150 bp, $KEYS + $KEYS 21-mers"
  tools/gen_fastq $D $NPAIRS $KEYS $NBC 21 150 $THREADS 0 > /dev/null || exit 1
  cat $D/r1.fq $D/r2.fq > /dev/null
  for mode in $MODES; do
    ARGS="--hap0 $D/hap0.mer --hap1 $D/hap1.mer --weight0 1.04 --thread $THREADS --stats --read $D/r1.fq --read $D/r2.fq"
    [ $mode = phase ] && ARGS="$ARGS --phase-reads"
    for i in $(seq 1 $RUNS); do
      run parent $mode $i $PARENT/classify || exit 1; P=$MD5; sleep $PAUSE
      run host $mode $i $NEW --rows host || exit 1; H=$MD5; sleep $PAUSE
      run device $mode $i $NEW --rows device || exit 1; V=$MD5; sleep $PAUSE
      [ "$P" = "$H" ] && [ "$P" = "$V" ] || { echo "-- $mode run $i: the three stdouts DIFFER ($P $H $V)"; exit 1; }
      if [ $mode = phase ]; then
        for f in paternal.unique.barcodes maternal.unique.barcodes homozygous.unique.barcodes filter_reads.log; do
          cmp -s $D/w.parent/$f $D/w.device/$f && cmp -s $D/w.host/$f $D/w.device/$f || { echo "-- $mode run $i: $f DIFFERS between the legs"; exit 1; }
        done
        echo "-- $mode run $i: the three stdouts are md5-equal, the three lists and filter_reads.log are the same bytes ($(cat $D/w.device/*.unique.barcodes | wc -c) bytes of lists)"
      else
        echo "-- $mode run $i: the three stdouts are md5-equal"
      fi
    done
    rm -rf $D/w.parent $D/w.host $D/w.device
  done
  echo "== $NBC barcodes: medians and ranges over $RUNS runs (table_s = counters_back_s + sort_print_s; with --phase-reads it holds lists_s and the routing)"
  python3 - $D/figures.$NBC <<'EOF'
import statistics, sys
fig = {}
for line in open(sys.argv[1]):
    leg, name, v = line.split()
    fig.setdefault((name, leg), []).append(float(v))
for (name, leg), v in sorted(fig.items()):
    print("%-14s %-8s median %.3f  range %.3f .. %.3f  (n = %d)" % (name, leg, statistics.median(v), min(v), max(v), len(v)))
EOF
  rm -f $D/*.fq $D/*.mer
done
echo "== done"
