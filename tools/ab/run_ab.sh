#!/bin/bash
# A/B several versions of rtk_trace.hip on the same MI355X box (hipcc codegen is sensitive to small source changes):
#   put candidate sources at tools/ab/<name>.hip, then gpurun -- tools/ab/run_ab.sh name1 name2 ...
# Each is built into its own library and timed on C2 next to the committed kernel (RTK_HIP_LIB override).
cd "$GRAFT_REPO_ROOT"
for n in "$@"; do
  mkdir -p gpurun_out/ab/$n
  cp tools/ab/$n.hip gpurun_out/ab/$n/rtk_trace.hip
  cand=$PWD/$_  # (the copy just made)
  # the library's own command line (__graft_entry__.hip_build_command) with the candidate in place of csrc/rtk_trace.hip
  $(python3 -c "import sys, shlex, __graft_entry__ as g; print(shlex.join(g.hip_build_command(sys.argv[2], sources=[sys.argv[1] if f == 'rtk_trace.hip' else f for f in g.HIP_SOURCES])))" $cand ${cand%/rtk_trace.hip}.so) &
done
wait
CFG=${AB_CONFIG:-c2}; SPP=${AB_SPP:-0}; REAL=${AB_REAL:-f64}
for i in 1 2; do
  for n in "$@"; do RTK_DEV_TOOLS=1 RTK_HIP_LIB=$PWD/gpurun_out/ab/$n.so python tools/render_once.py $CFG $REAL 3 $SPP | tail -1 | cut -c1-48 | sed "s/^/$n ($CFG): /"; done
  python tools/render_once.py $CFG $REAL 3 $SPP | tail -1 | cut -c1-48 | sed "s/^/current ($CFG): /"
done
