#!/usr/bin/env bash
# AddressSanitizer + UBSan over the host code of csrc/abi_gradop.hip (argument checks, buffer sizing), on a CPU: abi_gradop.hip and
# tools/sanitize_gradop_driver.hip -- a stand-alone program with its own main -- are compiled with the sanitizers on the HOST side only
# and linked with the library's other objects as `python -m ninpol_amd.build` left them.  No device is opened, nothing is loaded into
# Python, and the device code is not instrumented.
# Usage: bash tools/sanitize_gradop.sh [DRIVER.hip]     (exit code 0 = clean)
# DRIVER.hip: another stand-alone program of tools/ to build and run that way in its place (tools/launch_layer_driver.hip: the launch
# layer of csrc/launch.hpp, which is header code and so instrumented with the driver)
set -u -o pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
DRIVER="${1:-$ROOT/tools/sanitize_gradop_driver.hip}"
NAME="$(basename "$DRIVER" .hip)"
W="${TMPDIR:-/tmp}/nin_sanitize_gradop"
mkdir -p "$W"
ROCM="${ROCM_PATH:-/opt/rocm}"
HIPCC="$(command -v hipcc || echo "$ROCM/bin/hipcc")"
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer"
fail=0
( cd "$ROOT" && python -m ninpol_amd.build >/dev/null ) || fail=1
OBJ="$ROOT/ninpol_amd/csrc/_obj"
"$HIPCC" --offload-arch=gfx950 -O1 -g -fPIC -std=c++17 -Wno-unknown-pragmas $SAN -c "$ROOT/ninpol_amd/csrc/abi_gradop.hip" -o "$W/abi_gradop.o" || fail=1
"$HIPCC" --offload-arch=gfx950 -O1 -g -fPIC -std=c++17 -Wno-unknown-pragmas $SAN -c "$DRIVER" -o "$W/$NAME.o" || fail=1
others=$(ls "$OBJ"/*.o | grep -v -e /abi_gradop.o)
"$HIPCC" --offload-arch=gfx950 -fsanitize=address,undefined "$W/$NAME.o" "$W/abi_gradop.o" $others -L "$ROCM/lib" -lamdhip64 -lgomp \
    -Wl,-rpath,"$ROCM/lib" -o "$W/$NAME" || fail=1
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 "$W/$NAME" || fail=1
echo "== sanitizers: $([ $fail = 0 ] && echo CLEAN || echo FINDINGS)"
exit $fail
