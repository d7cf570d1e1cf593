#!/bin/sh
# sha256 of the gfx950 code object inside each given .o (what the GPU executes, without the host half of the object):
#   tools/codeobj_hash.sh gym-genesis_amd/csrc/mir_step.o gym-genesis_amd/csrc/mir_step_convex.o ...
# A refactor of the kernels' bookkeeping must leave these hashes as they were.  Reads .o files only; runs nothing on a GPU.
set -e
ROCM_LLVM=${ROCM_LLVM:-/opt/rocm/llvm/bin}
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
for o in "$@"; do
  "$ROCM_LLVM/llvm-objcopy" --dump-section .hip_fatbin="$tmp/fat.bin" "$o"
  "$ROCM_LLVM/clang-offload-bundler" --type=o --unbundle --input="$tmp/fat.bin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$tmp/x.co"
  printf '%s  %s\n' "$(sha256sum < "$tmp/x.co" | cut -d' ' -f1)" "$o"
done
