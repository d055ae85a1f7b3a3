#!/bin/bash
# developer helper: build a variant of libsmalfit.so from the current sources with extra compiler flags -- the instrumentation builds
# (-DSMALFIT_DEV_PROBES, -DSMALFIT_WORK_STATS, -DSMALFIT_PHASES), or no flags for a constant edited in a scratch branch.
# usage: tools/build_variant.sh NAME [FLAGS ...]
# run a tool against it with SMALFIT_LIB=smalify_amd/_variants/NAME.so
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p smalify_amd/_variants
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -fPIC -shared "$@" smalify_amd/csrc/smalfit_kernels.hip -o smalify_amd/_variants/$name.so
echo smalify_amd/_variants/$name.so
