#!/bin/bash
# ASan + UBSan build of the device write's host code (devdest.cpp) and a walk of the stand-alone entries' refusals (CPU only; the
# library must have been built: the request table sizes its destinations with it).  Prints "case | family: status message" per
# request; SRC=<dir> takes devdest.cpp and its headers from another tree (a checkout of the commit to compare with).
set -e -o pipefail
cd "$(dirname "$0")/../.."
S=${SRC:-heif-decoder-lib_amd/csrc}
OUT=${TMPDIR:-/tmp}/hm_asan_target_walk
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
    -Iinclude -I$S -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
    tools/asan/target_walk.cpp $S/devdest.cpp $S/devpool.cpp $S/colour_host.cpp $S/common.cpp \
    -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -Wl,--unresolved-symbols=ignore-all -lpthread -o $OUT
python3 tools/asan/target_walk.py | ASAN_OPTIONS=detect_leaks=0 $OUT
