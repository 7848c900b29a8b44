# run on the GPU box: the -m gpu suite, then short benches of c3 and the default (refseq) config, the latter with the output checks
# usage: bash scripts/quick_check.sh [tag] [output directory, default quick_check_out]
set -e
export TMPDIR=/tmp
T=${1:-quick}; O=${2:-quick_check_out}
mkdir -p $O
timeout -k 10 700 python -m pytest tests -m gpu -x -q > $O/${T}_pytest.log 2>&1
tail -3 $O/${T}_pytest.log
timeout -k 10 300 python3 bench.py --config c3 --steps 8 --warmup 3 > $O/${T}_c3.json 2> $O/${T}_c3.err
echo c3 done
timeout -k 10 400 python3 bench.py --steps 8 --warmup 3 --full --no-cpu-baseline > $O/${T}_refseq.json 2> $O/${T}_refseq.err
echo refseq done
