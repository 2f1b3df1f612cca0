#!/bin/bash
# AddressSanitizer + UBSan over the HOST code of libaar (file readers / writers, synthetic generator, shard planner, the
# Initializer's argument checking) with the device entry points stubbed -- GPU sanitizers are not available on this pool.
#   bash tests/tools/asan_host.sh      (from the repo root; prints the program's output, any sanitizer report fails it)
set -e
cd "$(dirname "$0")"
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
H=../../automatic-ar_amd/host
g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer asan_host_main.cpp \
    $H/dataset.cpp $H/synth.cpp $H/solution_io.cpp $H/cam_config.cpp $H/initializer.cpp -o "$T/asan_host"
mkdir "$T/files"
"$T/asan_host" "$T/files"
