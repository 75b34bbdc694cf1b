#!/bin/bash
# Build a variant of libvbm25.so whose scan_win.hip is compiled with extra flags (kernel experiments):
#   tools/win_variant.sh <name> [hipcc flags ...]   ->  vectorchord-bm25_amd/csrc/libvbm25_<name>.so
# Run it on the GPU box with VBM25_LIBRARY=$GRAFT_REPO_ROOT/vectorchord-bm25_amd/csrc/libvbm25_<name>.so python bench.py ...
set -e
cd "$(dirname "$0")/../vectorchord-bm25_amd/csrc"
name=$1; shift
make -s variant VARIANT="$name" UNIT=scan_win.hip EXTRA="$*"
echo built libvbm25_$name.so
