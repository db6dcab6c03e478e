# classify --phase-reads --gz-out --gz-format bgzf measured against its yardstick: the same generated reads routed
# and deflated on the GPU three ways, RUNS runs each, the legs alternating, PAUSE seconds between two processes:
#   parent   the parent commit's binaries ($PARENT: that commit's classify + libhast.so, built by hand, not committed) with --gz-out
#   gzip     this tree with --gz-out (ordinary members, one per routed run)
#   bgzf     this tree with --gz-out --gz-format bgzf (members of three pieces with a BC header, an end-of-file block per file)
# Per run: the routing phase's seconds (__stats_phase_reads__ routing_s), the bytes on disk and the __stats_route_gz__ lines.  Asserted:
# the three stdouts are md5-equal; the parent and gzip legs write the same bytes; per input the device-made bytes of the bgzf leg are
# those of the gzip leg + 28 a member - 20 a run, exactly (the pieces' bytes do not change); the files of the last runs inflate to the
# same bytes.  Then the summed time of the k_dz_ kernels of one run of each leg (rocprofv3 --kernel-trace --stats, runs of their own, no
# counters), and one written file read back: the bgzf leg's with --bgzf device against the gzip leg's on the ordinary device route.
# Every GPU step has its own time limit and the steps are chained: a step that fails or runs out of time ends the job.
# usage (on a box with an MI355X, after the build and `make -C tools gen_fastq`):
#   PARENT=dir bash tools/gpu/bgzf_out.sh > profiles/bgzf_out.txt 2>&1
#   NPAIRS (default 10000000: 20M reads in two files), KEYS (2000000), BARCODES (200000), RUNS (5), THREADS (16), PAUSE (3)
#   ORDER (default "parent gzip bgzf": the order of the legs inside a round), STEPS (default "time prof back": the timed rounds, the
#   kernel times, the read-back; prof and back need time)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
NPAIRS=${NPAIRS:-10000000}; KEYS=${KEYS:-2000000}; BARCODES=${BARCODES:-200000}; RUNS=${RUNS:-5}; THREADS=${THREADS:-16}; PAUSE=${PAUSE:-3}
ORDER=${ORDER:-parent gzip bgzf}; STEPS=${STEPS:-time prof back}
has() { case " $STEPS " in *" $1 "*) return 0;; esac; return 1; }
PARENT=$(cd "${PARENT:-tools/ab_old}" 2>/dev/null && pwd)
[ -n "$PARENT" ] && [ -x $PARENT/classify ] && [ -f $PARENT/libhast.so ] || { echo "PARENT: a directory with the parent commit's classify and libhast.so"; exit 1; }
D=$(mktemp -d /dev/shm/hast_bzo.XXXXXX)
( while sleep 45; do echo "[still running $(date +%T)]"; done ) &
HB=$!
trap 'kill $HB 2>/dev/null; rm -rf $D' EXIT
now() { date +%s.%N; }
el() { python3 -c "print(round($2-$1,2))"; }
NEW=$PWD/hast_amd/classify
echo "== box: cpu.max $(cat /sys/fs/cgroup/cpu.max 2>/dev/null), /dev/shm $(df -h /dev/shm | tail -1 | awk '{print $4}') free"
tools/gen_fastq $D $NPAIRS $KEYS $BARCODES 21 150 $THREADS 0 > /dev/null || exit 1
echo "== $((2 * NPAIRS)) reads of 150 bp: $(stat -c %s $D/r1.fq) + $(stat -c %s $D/r2.fq) bytes of FASTQ"
ARGS="--hap0 $D/hap0.mer --hap1 $D/hap1.mer --weight0 1.04 --thread $THREADS --stats --phase-reads --gz-out --read $D/r1.fq --read $D/r2.fq"
# one run: $1 = leg, $2 = run number, $3 = the program, the rest = the leg's flags; its files stay in $D/w.$leg until the leg's next run
run() { local leg=$1 i=$2 exe=$3; shift 3
  local w=$D/w.$leg; rm -rf $w; mkdir -p $w
  local t0=$(now)
  (cd $w && timeout -k 10 300 $exe $ARGS "$@" > out.tsv 2> err) || { echo "-- $leg run $i FAILED rc=$?"; tail -5 $w/err; return 1; }
  local t1=$(now)
  MD5=$(md5sum < $w/out.tsv | cut -c1-32)
  local routing=$(grep -h -o ' routing_s=[0-9.]*' $w/err | cut -d= -f2) disk=$(cat $w/*.fastq.gz | wc -c)
  echo "-- $leg run $i: whole process $(el $t0 $t1) s, $(grep -h -o 'lists_and_routing_s=[0-9.]* lists_s=[0-9.]* routing_s=[0-9.]*' $w/err) $(grep -h -o 'waiting_for_gpu_s=[0-9.]* idle_s=[0-9.]*' $w/err); bytes on disk $disk; stdout md5 $MD5"
  grep -h "^__stats_route_gz__" $w/err | sed 's/^/     /'
  echo "$leg routing_s $routing" >> $D/figures
  echo "$leg bytes_on_disk $disk" >> $D/figures
  grep -h "^__stats_route_gz__" $w/err | sed "s/^__stats_route_gz__/$leg/" > $D/route_gz.$leg
  return 0; }
has time || { echo "== STEPS without time: nothing to do"; exit 1; }
echo "== the legs of a round in the order: $ORDER"
for i in $(seq 1 $RUNS); do
  for leg in $ORDER; do
    case $leg in
      parent) run parent $i $PARENT/classify || exit 1; P=$MD5;;
      gzip) run gzip $i $NEW || exit 1; G=$MD5;;
      bgzf) run bgzf $i $NEW --gz-format bgzf || exit 1; B=$MD5;;
      *) echo "ORDER: parent, gzip and bgzf"; exit 1;;
    esac
    sleep $PAUSE
  done
  [ "$P" = "$G" ] && [ "$P" = "$B" ] || { echo "-- run $i: the three stdouts DIFFER ($P $G $B)"; exit 1; }
  # the sizes, per input: parent == gzip; bgzf - gzip == 28 * members - 20 * runs on the device-made bytes
  python3 - $D/route_gz.parent $D/route_gz.gzip $D/route_gz.bgzf <<'EOF' || exit 1
import sys
def lines(path):
    return [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in open(path)]
parent, gz, bz = (lines(p) for p in sys.argv[1:4])
assert len(parent) == len(gz) == len(bz) > 0
for p, g, b in zip(parent, gz, bz):
    assert p["file"] == g["file"] == b["file"] and b.get("format") == "bgzf" and "format" not in g
    for k in ("device_bytes_in", "device_bytes_out", "device_members", "host_bytes_in", "host_bytes_out", "host_members"):
        assert p[k] == g[k], (k, p[k], g[k])
    assert g["device_bytes_in"] == b["device_bytes_in"] and g["host_bytes_in"] == b["host_bytes_in"]
    runs, members = int(g["device_members"]), int(b["device_members"])
    extra = int(b["device_bytes_out"]) - int(g["device_bytes_out"])
    assert extra == 28 * members - 20 * runs, (extra, members, runs)
    print("     %s: %d runs -> %d members on the device, %d bytes more = 28 * members - 20 * runs (%.4f %% of %s); host: %s -> %s members" % (
        g["file"].split("/")[-1], runs, members, extra, 100.0 * extra / int(g["device_bytes_out"]), g["device_bytes_out"], g["host_members"], b["host_members"]))
EOF
  echo "-- run $i: the three stdouts are md5-equal, the sizes are as computed"
done
echo "== the files of the last runs, inflated (gzip -dc): md5 per file, the three legs side by side"
for f in $(cd $D/w.gzip && ls *.fastq.gz); do
  (gzip -dc $D/w.parent/$f | md5sum | cut -c1-32 > $D/md5.p & gzip -dc $D/w.gzip/$f | md5sum | cut -c1-32 > $D/md5.g & gzip -dc $D/w.bgzf/$f | md5sum | cut -c1-32 > $D/md5.b & wait)
  echo "   $f: $(cat $D/md5.p) $(cat $D/md5.g) $(cat $D/md5.b); $(stat -c %s $D/w.gzip/$f) bytes as gzip, $(stat -c %s $D/w.bgzf/$f) as bgzf"
  [ "$(cat $D/md5.p)" = "$(cat $D/md5.g)" ] && [ "$(cat $D/md5.p)" = "$(cat $D/md5.b)" ] || { echo "-- $f inflates to DIFFERENT bytes"; exit 1; }
  cmp -s $D/w.parent/$f $D/w.gzip/$f || { echo "-- $f: the gzip leg's bytes are not the parent's"; exit 1; }
done
echo "== medians and ranges over $RUNS runs"
python3 - $D/figures <<'EOF'
import statistics, sys
fig = {}
for line in open(sys.argv[1]):
    leg, name, v = line.split()
    fig.setdefault((name, leg), []).append(float(v))
for (name, leg), v in sorted(fig.items()):
    print("%-14s %-8s median %.3f  range %.3f .. %.3f  (n = %d)" % (name, leg, statistics.median(v), min(v), max(v), len(v)))
r = {leg: fig[("routing_s", leg)] for leg in ("parent", "gzip", "bgzf")}
for leg in ("gzip", "bgzf"):
    m = statistics.median(r[leg])
    inside = min(r["parent"]) <= m <= max(r["parent"])
    print("routing_s: the %s leg's median %.3f lies %s the parent leg's range %.3f .. %.3f (%+.1f %% against the parent's median)" % (
        leg, m, "within" if inside else "OUTSIDE", min(r["parent"]), max(r["parent"]), 100.0 * (m / statistics.median(r["parent"]) - 1)))
EOF
# the read-back inputs are kept, the rest of the written files goes
BIG=$(cd $D/w.gzip && ls -S r1.fq.*.fastq.gz | head -1)
mv $D/w.gzip/$BIG $D/back.gzip.fq.gz && mv $D/w.bgzf/$BIG $D/back.bgzf.fq.gz || exit 1
rm -rf $D/w.parent $D/w.gzip $D/w.bgzf
if has prof; then
echo "== summed time of the k_dz_ kernels, one run of each leg under rocprofv3 --kernel-trace --stats"
prof() { local leg=$1 exe=$2; shift 2
  local w=$D/prof.$leg; mkdir -p $w
  (cd $w && timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $w/out -o dz -- $exe $ARGS "$@" > out.tsv 2> err) || { echo "-- $leg profile run FAILED rc=$?"; tail -5 $w/err; return 1; }
  python3 - $leg $(find $w/out -name '*kernel_stats.csv' | head -1) <<'EOF'
import csv, sys
total = 0
for r in csv.DictReader(open(sys.argv[2])):
    name = r["Name"].split("(")[0]
    if "k_dz_" in name:
        total += int(r["TotalDurationNs"])
        print("   %-8s %-44s calls=%-6s total_ms=%-10.2f avg_us=%.1f" % (sys.argv[1], name[-44:], r["Calls"], int(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e3))
print("   %-8s k_dz_ kernels in all: %.2f ms" % (sys.argv[1], total / 1e6))
EOF
  rm -rf $w; return 0; }
prof parent $PARENT/classify && sleep $PAUSE && prof gzip $NEW && sleep $PAUSE && prof bgzf $NEW --gz-format bgzf || exit 1
sleep $PAUSE
fi
has back || { echo "== done"; exit 0; }
echo "== one written file read back ($BIG: $(stat -c %s $D/back.gzip.fq.gz) bytes as gzip, $(stat -c %s $D/back.bgzf.fq.gz) as bgzf): read_phase_s"
BACK="--hap0 $D/hap0.mer --hap1 $D/hap1.mer --weight0 1.04 --thread $THREADS --stats"
back() { local leg=$1 i=$2; shift 2
  timeout -k 10 300 $NEW $BACK "$@" > $D/out 2> $D/err || { echo "-- $leg run $i FAILED rc=$?"; tail -5 $D/err; return 1; }
  MD5=$(md5sum < $D/out | cut -c1-32)
  local phase=$(grep -o 'read_phase_s=[0-9.]*' $D/err | cut -d= -f2)
  echo "-- $leg run $i: read_phase_s $phase; md5 $MD5 $(grep -h -o '^__stats_bgzf__ file=[^ ]* members=[0-9]* batches=[0-9]*\|^__stats_gz__ file=[^ ]* compressed_bytes=[0-9]* inflated_bytes=[0-9]* chunks=[0-9]*' $D/err | sed 's/file=[^ ]* //')"
  echo "$leg read_phase_s $phase" >> $D/back_figures; return 0; }
for i in $(seq 1 $RUNS); do
  back gzip_device_route $i --read $D/back.gzip.fq.gz || exit 1; G=$MD5; sleep $PAUSE
  back bgzf_per_member $i --read $D/back.bgzf.fq.gz --bgzf device || exit 1; B=$MD5; sleep $PAUSE
  [ "$G" = "$B" ] || { echo "-- run $i: the two stdouts DIFFER"; exit 1; }
done
python3 - $D/back_figures <<'EOF'
import statistics, sys
fig = {}
for line in open(sys.argv[1]):
    leg, name, v = line.split()
    fig.setdefault(leg, []).append(float(v))
for leg, v in sorted(fig.items()):
    print("%-18s read_phase_s median %.3f  range %.3f .. %.3f  (n = %d)" % (leg, statistics.median(v), min(v), max(v), len(v)))
EOF
echo "== done"
