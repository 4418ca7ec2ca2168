#!/bin/bash
# Build an A/B variant of libplenum_verify.so with extra defines into variants/<name>/ (selected at
# run time with PLENUM_AMD_LIB=variants/<name>/libplenum_verify.so). Usage: build_variant.sh NAME -DX=1 ...
# Every source of the library's Makefile is compiled with the flags (its SRC is the one list of them).
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/variants/$name
make -s -j16 -C "$root/indy-plenum_amd" EXTRA="$*" BUILD="$out/build" OUT="$out/libplenum_verify.so" \
  "$out/libplenum_verify.so"
rm -rf "$out/build"
echo "$out/libplenum_verify.so"
