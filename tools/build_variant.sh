#!/bin/bash
# Build an A/B variant of the HIP library: tools/build_variant.sh NAME [extra hipcc flags...]
# -> 3d-renderer_amd/lib/variants/NAME.so (select it with TRI_RASTER_LIB=... on the GPU box).
# The Makefile builds it (its unit list, its per-unit flags, VERTEX_SCHED from the environment) into
# lib/variants/obj_NAME with the extra flags appended; every unit is recompiled, whatever is there already.
set -e
cd "$(dirname "$0")/../3d-renderer_amd"
name=$1; shift
make -B -j16 LIB=lib/variants/obj_$name EXTRA_HIPFLAGS="$*" lib/variants/obj_$name/libtri_raster.so
cp lib/variants/obj_$name/libtri_raster.so lib/variants/$name.so
echo "built lib/variants/$name.so"
