# stage 00: `unshared_kmers --ingest device` against `--ingest host` of the same tree and against another commit's binary run both ways (OLD=dir
# with that commit's libhast.so + unshared_kmers, built by hand, not committed; left out when there is none), on one box, alternating,
# 5 s apart (back-to-back processes lie).  Inputs: a tools/gen_trio trio of GENOME x COVERAGE bases per parent (default
# 50 Mbp x 40 = 2 Gbp) as plain FASTQ and as ONE gzip member per file (tools/pgzip1).  Every run has its own time limit and the chain
# ends at the first run that fails.  Writes profiles/s00_ingest.txt.
# Run from the repository root.
ROOT=$PWD
GENOME=${GENOME:-50000000}; COVERAGE=${COVERAGE:-40}; RUNS=${RUNS:-3}; OLD=${OLD:-}; TABLE_GB=${TABLE_GB:-48}; LIMIT=${LIMIT:-150}
D=$(mktemp -d ${TMPDIR:-/tmp}/s00_ingest.XXXXXX) || exit 1
trap 'rm -rf $D' EXIT
OUT=profiles/s00_ingest.txt
{
echo "# tools/gpu/s00_ingest.sh: genome $GENOME, coverage $COVERAGE per parent, table $TABLE_GB GB, $RUNS alternating runs per variant"
tools/gen_trio $D $GENOME $COVERAGE 150 1 16 || exit 1
for p in paternal maternal; do tools/pgzip1 $D/${p}_0.fq $D/${p}_0.fq.gz 6 16 || exit 1; done
ls -l $D | awk 'NR>1 {print "# " $5, $9}'
cat $D/*.fq $D/*.fq.gz > /dev/null
peak() { rocm-smi --showmeminfo vram --json 2>/dev/null | python3 -c "import json,sys; d=json.load(sys.stdin); print(max(int(v.get('VRAM Total Used Memory (B)',0)) for v in d.values())>>20)" 2>/dev/null; }
one() {   # name, exe, input suffix, extra args...
  local name=$1 exe=$2 suf=$3; shift 3
  mkdir -p $D/w && cd $D/w || return 1
  ( while sleep 1; do peak; done > $D/vram.txt ) & local mon=$!
  timeout -k 10 $LIMIT $exe --paternal $D/paternal_0.$suf --maternal $D/maternal_0.$suf --thread 8 --table-gb $TABLE_GB --stats "$@" > $D/out.txt 2> $D/err.txt; local rc=$?
  kill $mon 2>/dev/null; wait $mon 2>/dev/null
  cd - > /dev/null
  local t=$(grep -h "read+parse+count" $D/err.txt | sed 's/.*read+parse+count \([0-9.]*\) s.*total \([0-9.]*\) s.*/\1 \2/')
  local bases=$(grep -h "records, " $D/err.txt | sed 's/.* records, \([0-9]*\) bases.*/\1/' | awk '{s+=$1} END {print s+0}')
  local md5=$(cat $D/w/paternal.unique.filter.mer $D/w/maternal.unique.filter.mer 2>/dev/null | md5sum | cut -c1-12)
  echo "$name.$suf rc=$rc ingest_s=$(echo $t | cut -d' ' -f1) total_s=$(echo $t | cut -d' ' -f2) Gbp_per_s=$(python3 -c "print(round(${bases:-0}/1e9/max(${t%% *},1e-9),2))" 2>/dev/null) md5=$md5 vram_peak_MB=$(sort -n $D/vram.txt | tail -1) $(grep -h 'ingest device' $D/err.txt | cut -d' ' -f2-)"
  grep -h "hast_gz" $D/err.txt | sed 's/^/#   /'
  sleep 5
  return $rc
}
for suf in fq fq.gz; do
  for i in $(seq $RUNS); do
    if [ -n "$OLD" ]; then
      one old-host $OLD/unshared_kmers $suf --ingest host || exit 1
      one old-device $OLD/unshared_kmers $suf --ingest device || exit 1
    fi
    one host $ROOT/hast_amd/unshared_kmers $suf --ingest host || exit 1
    one device $ROOT/hast_amd/unshared_kmers $suf --ingest device || exit 1
  done
done
} 2>&1 | tee $OUT
