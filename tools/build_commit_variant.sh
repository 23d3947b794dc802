#!/bin/bash
# Build the HIP library of another commit as an A/B variant: tools/build_commit_variant.sh NAME COMMIT
# -> 3d-renderer_amd/lib/variants/NAME.so (select with TRI_RASTER_LIB=... on the GPU box). The commit's own sources
# and headers, built by the commit's own Makefile: its unit list and its flags, not this tree's.
set -e
cd "$(dirname "$0")/.."
name=$1; rev=$2
src=$(mktemp -d)
trap 'rm -rf "$src"' EXIT
out=$PWD/3d-renderer_amd/lib/variants
mkdir -p $out
git archive $rev 3d-renderer_amd include | tar -x -C $src
make -C $src/3d-renderer_amd -j16 lib/libtri_raster.so
cp $src/3d-renderer_amd/lib/libtri_raster.so $out/$name.so
echo "built 3d-renderer_amd/lib/variants/$name.so ($rev)"
