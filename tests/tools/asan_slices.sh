#!/bin/bash
# AddressSanitizer + UBSan over the host code, as tests/tools/asan_host.sh builds it (CPU only, the HIP layer stubbed out), on the
# streams whose slices differ in reference lists and loop-filter offsets: tests/tools/asan_slices.py.  Usage: tests/tools/asan_slices.sh
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd); out=${TMPDIR:-/tmp}/p264amd_asan_slices_$$
mkdir -p $out
objs=""
for f in parser vlc cabac dropin pipeline fanout input_layout compact cpu_check; do
  gcc -O1 -g -std=gnu11 -fPIC -fsanitize=address,undefined -fno-omit-frame-pointer -I$root/include -I$root/p264decoder_amd/csrc/host \
      -c $root/p264decoder_amd/csrc/host/$f.c -o $out/$f.o
  objs="$objs $out/$f.o"
done
gcc -O1 -g -fPIC -fsanitize=address,undefined -I$root/include -c $here/hip_stub.c -o $out/stub.o
gcc -shared -fsanitize=address,undefined -o $out/libp264amd_asan.so $objs $out/stub.o -lpthread
set -o pipefail
LD_PRELOAD=$(gcc -print-file-name=libasan.so) ASAN_OPTIONS=detect_leaks=0 python3 $here/asan_slices.py $out/libp264amd_asan.so 2>&1 | grep -v "^p264amd:" | tail -${ASAN_TAIL:-30}
rm -rf $out
