#!/bin/bash
# The host-side AddressSanitizer + UBSan build of the library (tools/host_asan_build.sh, shared with tools/host_asan.sh)
# and a run of tests/cpp/motion_args.cpp, tests/cpp/variance_args.cpp and tests/cpp/adaptive_args.cpp against it: the argument
# checks of vmx_motion_device, vmx_temporal_accumulate_motion_device, vmx_temporal_create_ex,
# vmx_temporal_accumulate_variance_device, vmx_filter_apply_variance_device and vmx_temporal_accumulate_adaptive_device,
# which are host code that runs before any device call.  Stand-alone programs; they need
# no GPU.       bash tools/host_asan_args.sh
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
. $R/tools/host_asan_build.sh
cd $R
for prog in motion_args variance_args adaptive_args; do
  /opt/rocm/lib/llvm/bin/clang++ -std=c++17 -g -fsanitize=address -fsanitize=undefined -fno-sanitize-recover=undefined -I include \
    tests/cpp/$prog.cpp build/libvermilion_hip_asan.so -Wl,-rpath,$R/build -o build/${prog}_asan
done
export ASAN_OPTIONS=detect_leaks=0:protect_shadow_gap=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1
./build/motion_args_asan
./build/variance_args_asan
./build/adaptive_args_asan
echo "host sanitizers: clean"
