# stage 00 on FASTA parents: `unshared_kmers --ingest device --device-fasta` against `--ingest host` and against `--ingest device`
# without the flag (a refusal and a restart through the host parser: what a tree without --device-fasta does too), on one box,
# alternating, 5 s apart (back-to-back processes lie).  Inputs: a tools/gen_trio trio of GENOME x COVERAGE bases per
# parent (default 50 Mbp x 40 = 2 Gbp) turned into two-line FASTA (fa), the same folded to 60 columns (fa60), and the two-line form as
# ONE gzip member per file (fa.gz, tools/pgzip1).  Every run has its own time limit and the chain ends at the first run that fails.
# Writes profiles/s00_ingest_fasta.txt.
# Run from the repository root.
ROOT=$PWD
GENOME=${GENOME:-50000000}; COVERAGE=${COVERAGE:-40}; RUNS=${RUNS:-3}; TABLE_GB=${TABLE_GB:-48}; LIMIT=${LIMIT:-150}
D=$(mktemp -d ${TMPDIR:-/tmp}/s00_ingest_fasta.XXXXXX) || exit 1
trap 'rm -rf $D' EXIT
OUT=profiles/s00_ingest_fasta.txt
{
echo "# tools/gpu/s00_ingest_fasta.sh: genome $GENOME, coverage $COVERAGE per parent, table $TABLE_GB GB, $RUNS alternating runs per leg"
tools/gen_trio $D $GENOME $COVERAGE 150 1 16 || exit 1
for p in paternal maternal; do
  awk 'NR % 4 == 1 { print ">" substr($0, 2) } NR % 4 == 2 { print }' $D/${p}_0.fq > $D/${p}_0.fa || exit 1
  awk 'NR % 4 == 1 { print ">" substr($0, 2) } NR % 4 == 2 { for (i = 1; i <= length($0); i += 60) print substr($0, i, 60) }' $D/${p}_0.fq > $D/${p}_0.fa60 || exit 1
  tools/pgzip1 $D/${p}_0.fa $D/${p}_0.fa.gz 6 16 || exit 1
  rm -f $D/${p}_0.fq
done
ls -l $D | awk 'NR>1 {print "# " $5, $9}'
cat $D/*.fa $D/*.fa60 $D/*.fa.gz > /dev/null
one() {   # name, input suffix, extra args...
  local name=$1 suf=$2; shift 2
  mkdir -p $D/w && cd $D/w || return 1
  timeout -k 10 $LIMIT $ROOT/hast_amd/unshared_kmers --paternal $D/paternal_0.$suf --maternal $D/maternal_0.$suf --thread 8 --table-gb $TABLE_GB --stats "$@" > $D/out.txt 2> $D/err.txt; local rc=$?
  cd - > /dev/null
  local t=$(grep -h "read+parse+count" $D/err.txt | sed 's/.*read+parse+count \([0-9.]*\) s.*total \([0-9.]*\) s.*/\1 \2/')
  local bases=$(grep -h "records, " $D/err.txt | sed 's/.* records, \([0-9]*\) bases.*/\1/' | awk '{s+=$1} END {print s+0}')
  local md5=$(cat $D/w/paternal.unique.filter.mer $D/w/maternal.unique.filter.mer 2>/dev/null | md5sum | cut -c1-12)
  echo "$name.$suf rc=$rc ingest_s=$(echo $t | cut -d' ' -f1) total_s=$(echo $t | cut -d' ' -f2) Gbp_per_s=$(python3 -c "print(round(${bases:-0}/1e9/max(${t%% *},1e-9),2))" 2>/dev/null) md5=$md5 $(grep -h 'ingest device' $D/err.txt | cut -d' ' -f2- | tr '\n' ' ')"
  grep -h "hast_gz" $D/err.txt | sed 's/^/#   /'
  sleep 5
  return $rc
}
for suf in fa fa60 fa.gz; do
  for i in $(seq $RUNS); do
    one host $suf --ingest host || exit 1
    one device-fasta $suf --ingest device --device-fasta || exit 1
    one device-noflag $suf --ingest device || exit 1
  done
done
} 2>&1 | tee $OUT
