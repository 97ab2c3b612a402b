#!/bin/bash
# sha256 of the unbundled gfx950 code object of every HIP unit of a source tree (device-only compile, the Makefile's flags): two trees whose lines are equal compile
# every kernel of those units to the same bytes.  (-fuse-cuid=none: the compilation-unit id the compiler otherwise derives from the source file's PATH, the one
# thing in a code object that differs between two copies of the same source.)  usage: tools/code_object_hashes.sh [tree]   (default: this one; a unit the tree does not have is left out)
TREE=$(cd "${1:-$(dirname "$0")/..}" && pwd)
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
# (the twelve kernel units of tools/kernel_resources.sh, the host driver and the GPU builder)
for UNIT in rf_renderer rf_bvh_gpu rf_shade rf_sums rf_trace rf_primary_lists rf_denoise rf_noise rf_robust rf_comm rf_checkpoint rf_features rf_ray_query rf_temporal; do
  [ -f "$TREE/rayfinder_amd/csrc/$UNIT.hip" ] || continue
  (
    /opt/rocm/bin/hipcc -std=c++20 -O3 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden --offload-arch=gfx950 -fhip-fp32-correctly-rounded-divide-sqrt \
      -fno-gpu-flush-denormals-to-zero -fuse-cuid=none -I"$TREE/include" --offload-device-only -c "$TREE/rayfinder_amd/csrc/$UNIT.hip" -o "$TMP/$UNIT.o" 2>/dev/null &&
    /opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$TMP/$UNIT.o" --output="$TMP/$UNIT.co" &&
    printf '%s  %s.hip  %s bytes\n' "$(sha256sum "$TMP/$UNIT.co" | cut -d' ' -f1)" "$UNIT" "$(stat -c %s "$TMP/$UNIT.co")" > "$TMP/$UNIT.line"
  ) &
done
wait
cat "$TMP"/*.line
