#!/bin/bash
# Build a variant of the HIP library for A/B runs (scripts/ab_bench.py):  scripts/build_variant.sh NAME [-DFLAG ...]
#   -> build/ab/libocc_NAME.so   (the hipcc command of __graft_entry__.build(), with the extra flags)
set -e
cd "$(dirname "$0")/.."
[ -n "$1" ] || { echo "usage: scripts/build_variant.sh NAME [-DFLAG ...]" >&2; exit 2; }
name=$1; shift
mkdir -p build/ab
python -c 'import subprocess, sys, __graft_entry__ as g; subprocess.check_call(g.hipcc_cmd(sys.argv[1], sys.argv[2:]))' \
  "$PWD/build/ab/libocc_$name.so" "$@"
echo "built build/ab/libocc_$name.so $*"
