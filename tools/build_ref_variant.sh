#!/bin/bash
# Build libdabgpu.so from a git revision's kernel sources for same-box A/B timing:
#   tools/build_ref_variant.sh NAME [REV]  ->  sdr-j-dab_amd/lib/variants/libdabgpu_NAME.so
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=${2:-HEAD}
TMP=$(mktemp -d)
git -C "$ROOT" archive "$REV" sdr-j-dab_amd/csrc sdr-j-dab_amd/host include | tar -x -C "$TMP"
P=$TMP/sdr-j-dab_amd
mkdir -p "$P/build" "$ROOT/sdr-j-dab_amd/lib/variants"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -w"
for f in $(cd "$P/csrc" && ls *.hip *.cpp); do      # whatever the layout holds (the revision's, for a ref variant)
    extra=""; [ "$f" = k_demod.hip ] && extra="-fno-slp-vectorize"
    { [ "$f" = k_audio.hip ] || [ "$f" = k_rate.hip ]; } && extra="-ffp-contract=off"      # (the Makefile's per-file flags)
    /opt/rocm/bin/hipcc $FLAGS $extra -x hip -c "$P/csrc/$f" -o "$P/build/$f.o" &
    pids="$pids $!"
done
for pid in $pids; do wait "$pid"; done                 # (set -e: a source that does not compile ends the build)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/sdr-j-dab_amd/lib/variants/libdabgpu_$1.so" "$P"/build/*.o
rm -rf "$TMP"
echo "$ROOT/sdr-j-dab_amd/lib/variants/libdabgpu_$1.so"
