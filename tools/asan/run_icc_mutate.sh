#!/bin/bash
# ASan + UBSan build of the ICC reader (csrc/icc.cpp) and a mutation run over writer-made seed profiles (CPU only, a stand-alone program).
set -e
cd "$(dirname "$0")/../.."
S=heif-decoder-lib_amd/csrc
OUT=${TMPDIR:-/tmp}/hm_asan_icc_mutate
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -ffp-contract=off \
    -Iinclude -I$S -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ \
    tools/asan/icc_mutate.cpp $S/icc.cpp $S/common.cpp \
    -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -lpthread -o $OUT
SEEDS=${TMPDIR:-/tmp}/hm_asan_icc_seeds
mkdir -p $SEEDS
python3 - "$SEEDS" <<'PY'
import sys
sys.path.insert(0, "tests")
import icc_cases
for name, data in icc_cases.all_profiles().items():
    open(f"{sys.argv[1]}/{name}.icc", "wb").write(data)
PY
ASAN_OPTIONS=detect_leaks=0 $OUT $SEEDS/*.icc "$@"
