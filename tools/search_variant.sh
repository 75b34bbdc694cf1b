#!/bin/bash
# Build a variant of libvbm25.so with one unit compiled with extra flags (kernel experiments outside scan_win.hip); the unit is
# search.hip, which holds the scan kernels, unless the first flag names another .hip file of csrc/:
#   tools/search_variant.sh <name> [unit.hip] [hipcc flags ...]   ->  vectorchord-bm25_amd/csrc/libvbm25_<name>.so
set -e
cd "$(dirname "$0")/../vectorchord-bm25_amd/csrc"
name=$1; shift
unit=search.hip
case "$1" in *.hip) unit=$1; shift;; esac
make -s variant VARIANT="$name" UNIT="$unit" EXTRA="$*"
echo built libvbm25_$name.so
