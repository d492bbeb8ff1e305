#!/bin/bash
# Diagnostic build of the device library with per-phase cycle stamps (-DSURTR_STAMP): build_tmp/libsurtr_hip_stamp.so
set -e
cd "$(dirname "$0")/.."
mkdir -p build_tmp
# every .hip and .cpp directly under csrc is a translation unit of the library (tests/test_source_list.py holds the build to that)
S=surtr_amd/csrc
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -fPIC -shared -DSURTR_STAMP "$@" -o build_tmp/libsurtr_hip_stamp.so \
    $S/*.hip $S/*.cpp
