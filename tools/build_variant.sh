#!/bin/bash
# Build an A/B variant of libtmhip.so from a copy of a whole tree, with that
# tree's own Makefile (so the source list and flags are the variant's own):
#   tools/build_variant.sh NAME [DIR|REV]  ->  build_ab/NAME/tmlibrary_amd/hip/libtmhip.so
# DIR: a directory holding a tree (its include/ and tmlibrary_amd/ are
# copied); REV: a git revision of this repository (git archive); neither:
# build_ab/NAME as it stands (a copy with some files swapped by hand).  Give the result to a bench run as TMH_LIB, or
# to tools/gpu.sh ab:R:LIB,LIB.
set -eu
NAME=$1
SRC=${2:-}
D=build_ab/$NAME
if [ -n "$SRC" ]; then
  mkdir -p "$D"
  if [ -d "$SRC" ]; then
    # what the library's build reads: the sources and the public headers
    tar -C "$SRC" --exclude=build --exclude='*.so' --exclude=__pycache__ -c include tmlibrary_amd \
      | tar -x -C "$D"
  else
    git archive "$SRC" | tar -x -C "$D"
  fi
fi
make -C "$D/tmlibrary_amd/csrc" -j"${JOBS:-16}"
ls -l "$D/tmlibrary_amd/hip/libtmhip.so"
