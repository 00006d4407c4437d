#!/bin/bash
# Build alternative libsnake_amd.so variants into marl-snake_amd/build/var/ for
# in-process A/B timing (scripts/ab_probe.py). Usage: build_variants.sh tag:flags ...
#   tag:flags   -> current sources compiled with extra flags (e.g. stamps:-DSNAKE_STAMPS)
#   tag@commit  -> the sources of a git commit, by that commit's own Makefile
# Every variant is one `make` of marl-snake_amd/csrc/Makefile with its own OUT
# and OBJ; the variants build side by side, each with JOBS (default 4) compilers.
# A tag is always built from scratch: its objects and library of an earlier call
# are removed first (make compares file times, not commits or flags).
set -eu
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/marl-snake_amd/build/var
mkdir -p "$OUT"
pids=""
for spec in "$@"; do
    if [[ $spec == *@* ]]; then
        tag=${spec%@*}; rev=${spec#*@}
        # (the commit's tree in the repository's own layout, so ../../include/ resolves)
        src=$OUT/src_$tag; rm -rf "$src"; mkdir -p "$src"
        paths=""; for p in marl-snake_amd/csrc include scripts/microbench; do
            git -C "$ROOT" cat-file -e "$rev:$p" 2>/dev/null && paths="$paths $p"
        done
        git -C "$ROOT" archive "$rev" $paths | tar -x -C "$src"
        # (ABI=n: an older commit's library under today's binding, which checks the version)
        if [[ -n ${ABI:-} ]]; then sed -i "s/define SNAKE_ABI_VERSION .*/define SNAKE_ABI_VERSION $ABI/" "$src/include/snake_env.h"; fi
        extra=""; dir=$src/marl-snake_amd/csrc
    else
        tag=${spec%%:*}; extra=${spec#*:}; dir=$ROOT/marl-snake_amd/csrc
        [[ $extra == "$spec" ]] && extra=""
    fi
    rm -rf "$OUT/obj_$tag" "$OUT/libsnake_$tag.so"
    make -s -C "$dir" -j"${JOBS:-4}" OUT="$OUT/libsnake_$tag.so" OBJ="$OUT/obj_$tag" EXTRA_FLAGS="$extra" &
    pids="$pids $!"
done
for p in $pids; do wait "$p"; done
ls -la "$OUT"/*.so
