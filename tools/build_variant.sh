#!/bin/bash
# tools/build_variant.sh TAG [-DMACRO=V ...] : builds circkit_amd/libcirckit_hip_TAG.so for tools/try_variants.sh
set -e
R=$(cd $(dirname $0)/.. && pwd)
tag=$1; shift
# the library's sources: circkit_amd/build.py HIP_SOURCES, the one list
srcs=$(cd $R && python3 -c "from circkit_amd.build import CSRC, HIP_SOURCES; print(' '.join(CSRC + '/' + s for s in HIP_SOURCES))")
hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC "$@" -o $R/circkit_amd/libcirckit_hip_$tag.so $srcs
