#!/bin/bash
# Full round-end style check: whole GPU test-suite, smoke, the bench with its --full extras, rocprofv3 kernel stats of the bench.
# usage: tools/gpu_full.sh OUT_DIR   (logs and the kernel-trace folder go to OUT_DIR)
OUT=$(mkdir -p "${1:?usage: tools/gpu_full.sh OUT_DIR}" && cd "$1" && pwd) || exit 1
export PYTHONUNBUFFERED=1 TMPDIR=/tmp
run() { name=$1; shift; echo "=== $name: $*"; timeout 1500 "$@" > $OUT/$name.log 2>&1; echo "rc=$? ($name)"; tail -n ${TAILN:-15} $OUT/$name.log; }
TAILN=6 run t_all python -m pytest tests -m gpu -q --tb=short
TAILN=3 run smoke python __graft_entry__.py --smoke
TAILN=2 run bench python bench.py --full
ROOTD=$(pwd); cd /tmp
timeout 900 rocprofv3 --kernel-trace --stats -d $OUT/prof_final -o bench -- python $ROOTD/bench.py --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/prof_final.log 2>&1
echo "rc=$? rocprof"; cd $ROOTD; ls -la $OUT/prof_final | head -5
