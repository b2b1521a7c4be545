#!/bin/bash
# build_variant.sh NAME [extra hipcc flags...] -> variants/NAME.so (for tools/ab.py A/B runs)
# The translation units are build.py's SOURCES, so a new one is listed once.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p variants
C=advancedgraphicsraytracer_amd/csrc
srcs=$(python3 -c "import sys; sys.path.insert(0, 'advancedgraphicsraytracer_amd'); import build; print(' '.join('$C/' + s for s in build.SOURCES))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -shared -Wno-unused-function \
  -I $C "$@" -o variants/$name.so -x hip $srcs -lz -ldl
echo variants/$name.so
