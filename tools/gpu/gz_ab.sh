# A/B of the device inflate of two trees on ONE box, in interleaved pairs: the tree's own binaries against those of another commit in
# ${AB_OLD:-tools/ab_old} (that commit's libhast.so + classify, built by hand, not committed): reads as two gzip -6 files, constant and
# noisy quality lines.  AB_READS (default 10000000) pairs per file, AB_REPS (3) pairs of runs per kind of quality line, AB_TESTS=0 skips the
# device inflate's tests in front, AB_PROF=0 the kernel statistics of one run of the tree behind.  Every run has a time limit of its own,
# and nothing more is started on the GPU after a run that was killed, aborted or hit its limit.
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
O=gpurun_out
mkdir -p $O
N=${AB_READS:-10000000}
REPS=${AB_REPS:-3}
if [ "${AB_TESTS:-1}" = 1 ]; then
  timeout -k 10 600 python -m pytest tests/test_gz_gpu.py -x -q > $O/gz_ab_pytest.log 2>&1; rc=$?; echo "pytest gz rc=$rc $(tail -1 $O/gz_ab_pytest.log)"
  [ $rc = 0 ] || { tail -30 $O/gz_ab_pytest.log; exit 1; }
fi
D=$(mktemp -d /tmp/hast_e2e.XXXXXX)
now() { date +%s.%N; }
run() { local name=$1; shift; local t0=$(now); timeout -k 10 ${AB_RUN_LIMIT:-300} "$@" > $D/out.$name 2> $D/err.$name; local rc=$?; local t1=$(now)
  echo "$name rc=$rc $(python3 -c "print(round($t1-$t0,3))") s md5=$(md5sum < $D/out.$name | cut -c1-12) $(grep -h __stats_phases__ $D/err.$name | grep -o "gpu_context_s=[0-9.]*\|read_phase_s=[0-9.]*\|total_s=[0-9.]*" | tr '\n' ' ') $(grep -h __stats_gz__ $D/err.$name | grep -o "decode_s=[0-9.]*" | tr '\n' ' ')"
  case $rc in 124|134|137|139) tail -5 $D/err.$name; rm -rf $D; exit 1;; esac; }
for q in const noisy; do
  if [ $q = noisy ]; then export GEN_FASTQ_QUAL=noisy; fi
  tools/gen_fastq $D $N $((N / 2)) 100000 21 150 16 0 || exit 1
  ARGS="--hap0 $D/hap0.mer --hap1 $D/hap1.mer --weight0 1.04"
  (gzip -6 -c $D/r1.fq > $D/r1.fq.gz & gzip -6 -c $D/r2.fq > $D/r2.fq.gz & wait)
  echo "== quality lines: $q; $(stat -c %s $D/r1.fq) bytes per file, $(stat -c %s $D/r1.fq.gz) as gzip -6"
  cat $D/r1.fq.gz $D/r2.fq.gz > /dev/null
  for rep in $(seq 1 $REPS); do
    run ${q}_new_$rep hast_amd/classify $ARGS --read $D/r1.fq.gz --read $D/r2.fq.gz -t 16 --stats
    run ${q}_old_$rep ${AB_OLD:-tools/ab_old}/classify $ARGS --read $D/r1.fq.gz --read $D/r2.fq.gz -t 16 --stats
  done
  if [ $q = const ] && [ "${AB_PROF:-1}" = 1 ]; then
    # the kernel statistics of one run of each tree (name, calls, total ns, average ns, ...: the inflate's kernels are the k_gz_ lines)
    for t in new:hast_amd old:${AB_OLD:-tools/ab_old}; do
      timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/gz_ab_prof_${t%%:*} -- ${t#*:}/classify $ARGS --read $D/r1.fq.gz --read $D/r2.fq.gz -t 16 --stats > $D/out.prof 2> $D/err.prof
      rc=$?
      echo "${t%%:*} under rocprofv3: rc=$rc md5=$(md5sum < $D/out.prof | cut -c1-12) $(grep -h __stats_phases__ $D/err.prof | cut -c1-300)"
      case $rc in 124|134|137|139) rm -rf $D; exit 1;; esac
      f=$(ls $O/gz_ab_prof_${t%%:*}/*/*kernel_stats.csv | head -1); head -1 $f; grep k_gz_ $f
    done
  fi
done
rm -rf $D
