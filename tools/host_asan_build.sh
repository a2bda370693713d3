# Host-side AddressSanitizer + UBSan build of the library into build/libvermilion_hip_asan.so (device code untouched:
# -fsanitize only after -Xarch_host).  Sourced by tools/host_asan.sh and tools/host_asan_args.sh with R = the repository's root.
mkdir -p $R/build
(cd $R/vermilion_amd/csrc && /opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -fPIC -ffp-contract=off -fno-slp-vectorize -Wno-unused-function \
  -DVMX_TRACE_WAVES_PER_SIMD=7 -DVMX_TRACE_SGPRS=80 -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer \
  -I$R/include -shared -o $R/build/libvermilion_hip_asan.so vmx_kernels.hip lbvh_build.hip path_compact.hip -x hip vmx_api.cpp bvh_build.cpp)
