# The batch geometry of classify --bgzf device: the same generated reads as blocked gzip through
# `classify --bgzf device --stats` at several batch sizes (HAST_BZ_BATCH_IN_BYTES / HAST_BZ_BATCH_OUT_BYTES), RUNS runs each, the
# settings taking turns.  Every GPU step has its own time limit and the steps are chained; PAUSE seconds lie between two processes.
# usage (on a box with an MI355X, after the build and `make -C tools gen_fastq to_bgzf`): bash tools/gpu/bgzf_geometry.sh > profiles/bgzf_geometry.txt 2>&1
#   NPAIRS (default 10000000), KEYS (5000000), BARCODES (100000), RUNS (3), THREADS (16), PAUSE (3), GEOMETRIES ("in_MB:out_MB ...")
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NPAIRS=${NPAIRS:-10000000}; KEYS=${KEYS:-5000000}; BARCODES=${BARCODES:-100000}; RUNS=${RUNS:-3}; THREADS=${THREADS:-16}; PAUSE=${PAUSE:-3}
GEOMETRIES=${GEOMETRIES:-"8:64 16:96 32:192 64:384"}
D=$(mktemp -d /dev/shm/hast_bz.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
EXE=$PWD/hast_amd/classify
tools/gen_fastq $D $NPAIRS $KEYS $BARCODES 21 150 $THREADS 0 > /dev/null || exit 1
for r in r1 r2; do
  tools/to_bgzf $D/$r.fq $D/$r.bgzf.fq.gz $THREADS 6 || exit 1
  rm -f $D/$r.fq
done
echo "== $((2 * NPAIRS)) reads of 150 bp as BGZF: $(stat -c %s $D/r1.bgzf.fq.gz) + $(stat -c %s $D/r2.bgzf.fq.gz) bytes"
ARGS="--hap0 $D/hap0.mer --hap1 $D/hap1.mer --weight0 1.04 --thread $THREADS --stats --bgzf device --read $D/r1.bgzf.fq.gz --read $D/r2.bgzf.fq.gz"
for i in $(seq 1 $RUNS); do
  for g in $GEOMETRIES; do
    IN=$(( ${g%%:*} << 20 )); OUT=$(( ${g##*:} << 20 ))
    t0=$(now)
    HAST_BZ_BATCH_IN_BYTES=$IN HAST_BZ_BATCH_OUT_BYTES=$OUT timeout -k 10 300 $EXE $ARGS > $D/out 2> $D/err || { echo "-- $g run $i FAILED rc=$?"; tail -5 $D/err; exit 1; }
    t1=$(now)
    echo "-- in:out MB $g run $i: whole process $(el $t0 $t1) s, read_phase_s $(grep -o 'read_phase_s=[0-9.]*' $D/err | cut -d= -f2), md5 $(md5sum < $D/out | cut -c1-12)"
    grep -h "^__stats_bgzf__" $D/err | sed 's/ file=[^ ]*//; s/^/     /'
    sleep $PAUSE
  done
done
echo "== done"
