#!/bin/bash
# Is a kernel of two builds of the HIP library the same code?  Extracts the gfx950 code object of both libraries, disassembles every kernel whose (mangled) name
# contains <kernel>, strips addresses and encodings, and diffs.  The symbol's own address line differs when code before it changed size; anything else is a change.
# Usage: tools/kernel_isa_diff.sh <a/libsigmaenv.so> <b/libsigmaenv.so> <kernel>     (e.g. sigmaenv_eval_accumulate_kernel; the parent's library: build a checkout of it)
set -e -o pipefail
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
[ $# -eq 3 ] || { sed -n 2,4p "$0"; exit 2; }
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
k=0
for lib in "$1" "$2"; do
  k=$((k + 1))
  $LLVM/llvm-objcopy --dump-section .hip_fatbin=$tmp/fat$k.bin "$lib" $tmp/copy$k.so
  $LLVM/clang-offload-bundler --unbundle --type=o --input=$tmp/fat$k.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/co$k.elf
  syms=$($LLVM/llvm-readelf -s --wide $tmp/co$k.elf | awk '$4 == "FUNC" {print $8}' | grep -F "$3" | grep -v '\.kd$' | sort -u | paste -sd, -)
  [ -n "$syms" ] || { echo "no kernel named *$3* in $lib" >&2; exit 1; }
  $LLVM/llvm-objdump -d --no-show-raw-insn --disassemble-symbols="$syms" $tmp/co$k.elf | sed '/file format/d; s/^ *//; s/ *\/\/ [0-9A-F]*:.*$//' > $tmp/k$k.s
  echo "$lib: $syms ($(grep -c . $tmp/k$k.s) lines)"
done
diff $tmp/k1.s $tmp/k2.s && echo "identical"
