#!/bin/bash
# Builds tests/san/leaf_group_san.cpp with the library's host sources and the host-only harness under AddressSanitizer +
# UndefinedBehaviorSanitizer and runs it.  CPU only (no device code, no GPU); see the program's head comment.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
CSRC="$ROOT/firewheel_amd/csrc"
H="$ROOT/tests/host_harness"
OUT="${1:-$(mktemp -d)/leaf_group_san}"
SRCS=$(sed -n 's/^SRCS *:= *//p' "$CSRC/Makefile" | tr ' ' '\n' | grep '\.cpp$' | sed "s|^|$CSRC/|")
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unused-function \
    -I "$H/fakehip" -I "$ROOT/include" -o "$OUT" "$ROOT/tests/san/leaf_group_san.cpp" "$H/launch_stubs.cpp" $SRCS
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$OUT"
