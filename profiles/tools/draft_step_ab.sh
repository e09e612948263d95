#!/bin/bash
# The seven draft-step bench scripts of a checkout of the parent commit (built, at scratch/parent) and of this tree in alternation -- parent, branch,
# parent, branch, parent -- each against its own profiles/tools/ab_build.sh library (name "parent" there, "branch" here); outputs under $AB_OUT.
# profiles/tools/draft_step_ab_table.py turns them into profiles/draft_step_ab.txt.
set -e -o pipefail
mkdir -p ${AB_OUT:-scratch/ab_runs}
run() {  # <tree> <lib name> <tag>
  local tree=$1 lib=$2 out=$PWD/${AB_OUT:-scratch/ab_runs}/${x%.py}.$3.txt
  shift 3
  if [ "$x" = conn_host_time.py ]; then
    SPECKV_LIB_PATH=$PWD/$tree/scratch/ab/$lib/libcxlspeckv.so timeout -k 10 400 python $tree/profiles/tools/$x > $out 2>&1
  else
    SPECKV_LIB_PATH=$PWD/$tree/scratch/ab/$lib/libcxlspeckv.so timeout -k 10 400 python $tree/profiles/tools/$x --out $out "$@" > /dev/null 2>&1
  fi
  echo "$x $out done: $(wc -l < $out) lines"
}
for x in k8v4_spec_bench.py k8v4_spec_wide_bench.py k8v4_layers_bench.py fp8_spec_window_bench.py fp8_spec_wide_bench.py mx4_spec_bench.py conn_host_time.py; do
  run scratch/parent parent parent1
  run . branch branch1
  run scratch/parent parent parent2
  run . branch branch2
  run scratch/parent parent parent3
done
