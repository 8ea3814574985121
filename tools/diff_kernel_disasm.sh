#!/bin/bash
# Machine code of the shipped kernels, before and after a change: tools/diff_kernel_disasm.sh <git-rev> (against the working tree)
# Compiles rt_device.hip and rt_multi.hip of both trees for gfx950 (device code only, the flags of csrc/Makefile), disassembles them
# with llvm-objdump -d and diffs the text, then diffs the per-kernel resource remarks (VGPRs, SGPRs, scratch, occupancy).
# Needs no GPU.  Exit status 0 = identical.
set -eu
rev=${1:?usage: tools/diff_kernel_disasm.sh <git-rev>}
root=$(git rev-parse --show-toplevel)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir -p "$tmp/a" "$tmp/b"
git -C "$root" archive "$rev" ray-tracing-v06_amd/csrc include | tar -x -C "$tmp/a"
(cd "$root" && tar -cf - ray-tracing-v06_amd/csrc include) | tar -x -C "$tmp/b"
FLAGS="-std=c++17 -O3 -fPIC -Wall -Wno-unused-function -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
       -fno-gpu-flush-denormals-to-zero -fno-fast-math -fno-slp-vectorize"
status=0
for side in a b; do
  for src in rt_device rt_multi; do
    (cd "$tmp/$side/ray-tracing-v06_amd/csrc" && /opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS -I../../include -I. \
        --cuda-device-only --no-gpu-bundle-output -Rpass-analysis=kernel-resource-usage -c $src.hip -o "$tmp/$side.$src.co" \
        2> "$tmp/$side.$src.res")
    /opt/rocm/llvm/bin/llvm-objdump -d --no-show-raw-insn "$tmp/$side.$src.co" | tail -n +3 > "$tmp/$side.$src.dis"
    grep "remark: " "$tmp/$side.$src.res" | sed 's/^.*remark: //' > "$tmp/$side.$src.usage"
  done
done
for src in rt_device rt_multi; do
  n=$(grep -c '^[0-9a-f]* <' "$tmp/b.$src.dis" || true)
  if diff -q "$tmp/a.$src.dis" "$tmp/b.$src.dis" > /dev/null && diff -q "$tmp/a.$src.usage" "$tmp/b.$src.usage" > /dev/null; then
    echo "$src: $n kernels, disassembly and resource usage identical"
  else
    echo "$src: DIFFERS"; diff "$tmp/a.$src.dis" "$tmp/b.$src.dis" | head -20 || true; diff "$tmp/a.$src.usage" "$tmp/b.$src.usage" | head -20 || true
    status=1
  fi
done
exit $status
