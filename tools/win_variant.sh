#!/bin/bash
# Build a variant of libvbm25.so whose scan_win.hip is compiled with extra flags (kernel experiments):
#   tools/win_variant.sh <name> [hipcc flags ...]   ->  vectorchord-bm25_amd/csrc/libvbm25_<name>.so
# Run it on the GPU box with VBM25_LIBRARY=$GRAFT_REPO_ROOT/vectorchord-bm25_amd/csrc/libvbm25_<name>.so python bench.py ...
set -e
cd "$(dirname "$0")/../vectorchord-bm25_amd/csrc"
name=$1; shift
others="search.o flush.o maintain.o pages_device.o pages_write.o resolve.o cast.o evaluate.o rerank.o segment.o pages.o blake3.o"
make -s $others >/dev/null 2>&1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -pthread -w "$@" -c scan_win.hip -o scan_win_$name.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o libvbm25_$name.so scan_win_$name.o $others
echo built libvbm25_$name.so
