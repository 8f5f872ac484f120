#!/bin/bash
# Build A/B variants of libmte.so into build_var/<name>/ (experiments only; the
# product library is fluidframework_amd/_lib/libmte.so).  The flat-pass
# and chunk-pass translation units are rebuilt with the variant's flags and
# linked with the product's other objects (make -C fluidframework_amd/csrc first).
# The knobs are the build-time macros of mte_replay.h (MTE_BURST, MTE_PASS1_EMAX)
# and the diagnostic switches of the other passes.  Pass 1's waves per SIMD are
# set per instantiation (pair_waves, mte_pass_pair.hip), not by a macro.  The rejected
# kernels DESIGN.md §6 measures (mte_lean.h, mte_rsmall.h) are not in the tree:
# tools/variants/ held them last at commit 58eea73.
# Usage: variants.sh name:"flags" ...   e.g. variants.sh w5e2:"-DMTE_PASS1_EMAX=2"
set -e
cd "$(dirname "$0")/.."
OBJ=fluidframework_amd/_lib/obj
PAIR_FLAGS=$(make -s -C fluidframework_amd/csrc pair-flags)
rm -rf build_var
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  mkdir -p build_var/$name
  ( /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 $flags -c \
      -o build_var/$name/flat.o fluidframework_amd/csrc/mte_pass_flat.hip &&
    # pass 1's unit with the product build's own option for it
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 $PAIR_FLAGS $flags -c \
      -o build_var/$name/pair.o fluidframework_amd/csrc/mte_pass_pair.hip &&
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 $flags -c \
      -o build_var/$name/chunk.o fluidframework_amd/csrc/mte_pass_chunk.hip &&
    /opt/rocm/bin/hipcc -O3 -fPIC --offload-arch=gfx950 -shared -o build_var/$name/libmte.so \
      $OBJ/mte_engine.o $OBJ/mte_pass_tree.o $OBJ/mte_pass_htree.o build_var/$name/pair.o build_var/$name/flat.o build_var/$name/chunk.o \
      $OBJ/mte_query.o $OBJ/mte_build.o \
      -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib ) &
done
wait
ls -la build_var/*/libmte.so
