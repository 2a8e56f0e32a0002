#!/bin/bash
# Build A/B variants of the kernel library HERE (hipcc cross-compiles gfx950 without a GPU); the .so files travel
# to the GPU box with the snapshot (tools/ab/build/*.so is git-ignored, not gpurun-ignored).
#   tools/ab/build_local.sh name1:"-DRTK_PROFILE" name2:"-DRTK_DEV_MASK_OFF=64u -DRTK_DEV_ONLY_ALL" plain: ...
cd "$(dirname "$0")/../.."
mkdir -p tools/ab/build
for spec in "$@"; do
  n=${spec%%:*}; flags=${spec#*:}; [ "$flags" = "$spec" ] && flags=""
  # the library's own command line (sources, flags) comes from __graft_entry__.hip_build_command
  $(python3 -c "import sys, shlex, __graft_entry__ as g; print(shlex.join(g.hip_build_command(sys.argv[1], sys.argv[2].split())))" tools/ab/build/$n.so "$flags") &
done
wait
ls -la tools/ab/build
