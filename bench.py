#!/usr/bin/env python3
"""bench.py -- the headline measurement: Msamples/s of the camera::render() sample
loop on the RTIOW book-1 final scene, 1920x1080x100 spp, depth 50 (BASELINE.json
configs[1]), on N MI355X GPUs of one node.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run does only what the headline needs: it sets up the scene, warms up, times the K steps, writes the
last timed step's outputs if --dump-outputs is given, and prints the result line (metric, value, unit,
higher_is_better, dtype, ms_per_step = milliseconds of one timed step).  Everything else below -- the pinned
framebuffer digest, the other visiting order, the roofline and its measured ceilings, the f32 mode (--f32), the
other BASELINE configs, the CPU baseline and, on N > 1, the C ABI multi-GPU path -- runs only with --full, where
the --no-* options still switch parts of it off.

--dump-outputs DIR: the arrays a caller of the timed path receives from its last timed step, as DIR/<name>.npy:
image.npy, the linear framebuffer (float64, H x W x 3), and rgb8.npy, the 8-bit image (as float32).  The files
stay within 64 MB in all: an array that does not fit in full is written as a fixed, seeded sample of its pixels
(<name>_sample.npy, one row per pixel, and <name>_sample_pixels.npy, their row-major indices as float64).

A "step" is one full render of the image: every rank renders its interleaved 8x8
tiles (no collective while rendering), then ONE gather of the compact tile buffers
to rank 0 over RCCL/xGMI and the un-permute kernel there.  The gather of frame k runs
while frame k+1 renders (two tile buffers per rank, tiling.GatherPipeline); all K frames
are rendered, gathered and un-permuted inside the timed region (--sync-gather: each frame
is gathered before the next one starts).  On several GPUs frames alternate between two
contexts on two streams (--frames-in-flight 2), so that the end of frame k -- a few long paths
on otherwise idle CUs, a sixth of an eighth of the frame -- overlaps the start of frame k+1;
every context renders one untimed frame first (it learns its tile hand-out order from it).
On one GPU the default is one stream (the overlap is worth 1 % there, and kernel durations
in a rocprofv3 trace of the command stay those of single launches).  Inputs (scene, camera)
are resident in HBM before the timed region; the framebuffer stays on the device.
value = W*H*spp*K / max-over-ranks(time) / 1e6, whole job.  Total work is fixed as
N grows, so scaling is "strong".

Visiting order: by default ("--order auto") the scene is rendered in the fast order of
rtk_scene_optimize (same primitives, SAH grouping, fewer aabb::hit calls per ray) when
the pass reports it bit-identical to the reference's bvh_node order -- it does for every
BASELINE config: exact ties follow the reference's visiting ranks, constant media keep
their positions in the reference's order -- otherwise in the reference order.  With --full the
other order is rendered too, outside the timed region, and reported under "other_order" with
its own rate; when the fast order claims exactness the two framebuffers must be
byte-identical or the run fails.

The headline dtype is f64: the reference computes in double (vec3.h:7) and the
parity bar (RMSE < 1e-4 against the CPU at matched seed) is only meaningful at
that precision.  The f32 kernels (statistical parity only) are timed
on request (--f32) and reported under "f32_mode" -- never as `value`.

Launching: `python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts
its own N ranks (a `python -m torch.distributed.run` child process, spawned before this
process imports torch or touches the GPU) and forwards rank 0's JSON line and exit code.

Extra objects on the JSON line (null unless --full):
  roofline      what bounds the render kernel is VALU issue on partially filled waves, not
                HBM (the program is served from LDS: measured HBM traffic is < 1 % of peak).
                bound = "valu"; achieved = VALU pipe-cycles the launch consumed per second
                (sum over instruction classes of wave-instructions x issue cycles: 2 for
                an f32-class, 4 for an f64 wave64 instruction on a SIMD-32) / kernel time;
                peak = SIMDs x clock; frac = achieved / peak <= 1, with the lane utilisation
                beside it.  Kernel time is measured live with HIP events on the launch
                stream; the instruction counts and HBM bytes come from rocprofv3 --pmc
                passes over THIS command (tools/pmc_collect.sh -> profiles/<round>_pmc_<config>.json),
                accepted only if that file names the same kernel, workload and kernel-source
                hash -- a stale file is refused and frac is null.  The SURVEY 8(d)
                algorithmic-byte model is reported under roofline.hbm_model (a model of bytes
                touched, served from LDS -- not a fraction of anything).
  cpu_baseline  the reference's own classes (oracle/_ref, kind "reference") or the
                CPU restatement (kind "port") timed on this box's host cores on a
                bounded sample of the same workload.  Rank 0, N=1 only.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 achievable
N_SIMDS = 256 * 4      # 256 CUs x 4 SIMD-32 (MI355X_MICROARCH.md, chip-level parameters)
MAX_CLOCK_GHZ = 2.4    # max shader clock; the clock held during the profiled launch is GRBM_GUI_ACTIVE / 8 / kernel time
PMC_ROUND = "r03"
WORKLOAD_NOTES = {"c4": "; the mesh is a procedural 1280-triangle stand-in for the reference's monkey.obj (a data asset that cannot travel to the GPU box, SURVEY 8(d))",
                  "c5": "; the earth texture is a procedural 1024x512 RGB8 stand-in for earthmap.jpg"}
# what the render kernel and the program it executes are built from (rtk_multi.cpp / rtk.h only route calls: not part of the key)
# Full-size framebuffer digests (f64 linear image, sha256[:16]) of the BASELINE configs at the committed seeds; the same
# constants are asserted by tests/test_gpu_parity.py against oracle-probed renders (the same values as round 2's driver run).
PINNED_SHA256 = {"c2": "02cec6778ff20839", "c3": "626eb89c5adf83ce", "c4": "d65a1ee77210444b", "c5": "5f3398426c23599e"}
KERNEL_SOURCES = ("raytracingoneweekendapplication_amd/csrc/rtk_trace.hip", "raytracingoneweekendapplication_amd/csrc/rtk_api.cpp",
                  "raytracingoneweekendapplication_amd/csrc/rtk_optimize.cpp", "raytracingoneweekendapplication_amd/csrc/rtk_device_layout.h",
                  "raytracingoneweekendapplication_amd/csrc/rtk_trace.h")


def kernel_source_hash():
    """Identifies the kernel code a PMC profile was taken on: sha256 over the sources librtk_hip.so is built from."""
    import hashlib

    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def load_pmc(config, kernel, workload, n_gpus):
    """The rocprofv3 --pmc record of this config's timed kernel (tools/pmc_collect.sh), or (None, reason) when there is
    none for exactly this kernel, workload and kernel-source hash."""
    path = os.path.join(ROOT, "profiles", f"{PMC_ROUND}_pmc_{config}.json")
    if not os.path.exists(path):
        return None, f"no profiles/{PMC_ROUND}_pmc_{config}.json"
    try:
        rec = json.load(open(path))
    except Exception as exc:
        return None, f"unreadable {path}: {exc}"
    want = {"kernel": kernel, "workload": workload, "n_gpus": n_gpus, "source_hash": kernel_source_hash()}
    for key, val in want.items():
        if rec.get(key) != val:
            return None, f"stale profiles/{PMC_ROUND}_pmc_{config}.json: {key} is {rec.get(key)!r}, this run has {val!r}"
    return rec, os.path.relpath(path, ROOT)


NOMINAL_ISSUE_CYCLES = {"f32": 2.0, "f64": 4.0, "trans_f32": 8.0, "trans_f64": 16.0, "mul_i32": 8.0}  # = tools/isa_costs.py NOMINAL_CYCLES


def issue_cycles(measured=None):
    """SIMD cycles a wave64 instruction of each class occupies the VALU issue for: measured on this box by
    csrc/rtk_microbench.hip (AGGREGATE rates: all wave instructions of a launch / SIMDs / its duration in cycles of the in-kernel
    clock, 8 independent chains per lane, 8 waves per SIMD) or, when no measurement is at hand, the nominal figures
    (MI355X_MICROARCH.md: v_fma_f32 2; f64 at half rate; transcendentals 4x)."""
    if not measured or not measured.get("issue_v_fma_f32", 0) > 0:
        return dict(NOMINAL_ISSUE_CYCLES), "nominal (MI355X_MICROARCH.md)"
    # The roofline's peak is the SPEC rate: one v_fma_f32 per 2 cycles per SIMD at 2.4 GHz.  v_fma_f32 is anchored at those 2
    # cycles and every other class is priced by its measured rate RELATIVE to the measured v_fma_f32 rate (a dense stream of
    # independent v_fma_f32 sustains ~0.45 per cycle on this chip, not 0.5: ceilings.issue_v_fma_f32_by_waves_per_simd; the
    # fraction of THAT ceiling is reported beside frac as frac_of_measured_issue_ceiling).
    anchor = NOMINAL_ISSUE_CYCLES["f32"] * measured["issue_v_fma_f32"]
    cost = lambda key: anchor / measured[key] if measured.get(key, 0) > 0 else None
    trans64 = [v for v in (cost("issue_v_rcp_f64"), cost("issue_v_rsq_f64"), cost("issue_v_sqrt_f64")) if v]
    trans32 = [v for v in (cost("issue_v_rcp_f32"), cost("issue_v_sqrt_f32")) if v]
    f64 = [v for v in (cost("issue_v_fma_f64"), cost("issue_v_mul_f64"), cost("issue_v_add_f64")) if v]
    got = {"f32": NOMINAL_ISSUE_CYCLES["f32"], "f64": sum(f64) / len(f64) if f64 else None, "trans_f32": sum(trans32) / len(trans32) if trans32 else None,
           "trans_f64": sum(trans64) / len(trans64) if trans64 else None, "mul_i32": cost("issue_v_mul_lo_u32")}
    return ({k: (round(v, 3) if v else NOMINAL_ISSUE_CYCLES[k]) for k, v in got.items()},
            "measured relative to v_fma_f32 = 2 cycles (csrc/rtk_microbench.hip, this run)")


def work_roofline(counters, isa, cycles, kernel_ms, spp_chunk=8):
    """roofline.work_frac: the VALU issue time the FRAME'S WORK needs at full lanes / the issue time the launch had.
    Numerator: exact work counters of the timed kernel's counting build x the instruction cost of each unit of work read from
    the ISA (tools/isa_costs.py: a box step, a sphere test, the start of a segment / a sample, a miss, a surface interaction
    priced at the CHEAPEST of the three materials, a partial-sum store per (pixel, chunk)), priced per class with `cycles`,
    / 64 lanes.  Denominator: 1024 SIMDs x 2.4 GHz x kernel time.  Executing more instructions, or the same ones on emptier
    waves, cannot raise it -- it is the fraction of the machine's VALU issue capacity that the necessary arithmetic of the
    algorithm as implemented would occupy."""
    cost = {k: sum(v[c] * cycles[c] for c in ("f32", "f64", "trans_f32", "trans_f64", "mul_i32")) for k, v in isa["costs"].items()}
    hit = min(cost["lambertian"], cost["metal"], cost["dielectric"])
    n = counters
    units = {"box_step": (n["box_tests"], cost["box"]), "sphere_test": (n["sphere_tests"], cost["sphere"]), "segment_start": (n["segments"], cost["segment"]),
             "sample_start": (n["samples"], cost["sample"]), "surface_hit_cheapest_material": (n["surface_hits"], hit),
             "miss": (n["segments"] - n["surface_hits"], cost["miss"]), "partial_sum_store": (n["samples"] / float(spp_chunk), cost["partial"])}
    lane_cycles = sum(w * c for w, c in units.values())          # SIMD cycles if every step ran on a wave of its own
    needed = lane_cycles / 64.0                                  # ... on full waves
    available = N_SIMDS * MAX_CLOCK_GHZ * 1e9 * kernel_ms * 1e-3
    return {"work_frac": round(needed / available, 4),
            "work_simd_cycles_per_sample": round(needed / n["samples"], 2),
            "work_by_unit_share": {k: round(w * c / lane_cycles, 4) for k, (w, c) in units.items()},
            "step_cost_simd_cycles": {k: round(v, 1) for k, v in cost.items()}}


def load_isa_costs():
    """profiles/<round>_isa_costs.json (tools/isa_costs.py --write), accepted only for the kernel sources it was derived from."""
    path = os.path.join(ROOT, "profiles", f"{PMC_ROUND}_isa_costs.json")
    if not os.path.exists(path):
        return None, f"no profiles/{PMC_ROUND}_isa_costs.json"
    rec = json.load(open(path))
    if rec.get("source_hash") != kernel_source_hash():
        return None, f"stale profiles/{PMC_ROUND}_isa_costs.json: derived from sources {rec.get('source_hash')!r}, this run has {kernel_source_hash()!r}"
    return rec, os.path.relpath(path, ROOT)


def valu_roofline(rec, kernel_ms, cycles=None, fma_by_waves=None):
    """VALU-issue roofline from PMC instruction counts (per launch) and the live kernel time.
    A CDNA4 SIMD is 32 lanes wide: a wave64 f32-class instruction occupies the pipe for 2 cycles, an f64 one for 4
    (MI355X_MICROARCH.md: vector FP64 peak = half the FP32 peak; v_fma_f32 wave64 = 2 cycles on a SIMD-32); with `cycles`
    (issue_cycles(): measured per class on this box) the f64 transcendentals (v_rcp / v_rsq / v_sqrt_f64) and the f32 ones are
    priced at their own rates instead of the plain 4 / 2."""
    c = rec["counters"]
    cycles = cycles or {"f32": 2.0, "f64": 4.0, "trans_f32": 2.0, "trans_f64": 4.0}
    trans64, trans32 = c.get("SQ_INSTS_VALU_TRANS_F64", 0), c.get("SQ_INSTS_VALU_TRANS_F32", 0)
    plain64 = c["SQ_INSTS_VALU_ADD_F64"] + c["SQ_INSTS_VALU_MUL_F64"] + c["SQ_INSTS_VALU_FMA_F64"]
    f64 = plain64 + trans64
    valu = c["SQ_INSTS_VALU"]
    pipe_cycles = cycles["f64"] * plain64 + cycles["trans_f64"] * trans64 + cycles["trans_f32"] * trans32 + cycles["f32"] * (valu - f64 - trans32)
    seconds = kernel_ms * 1e-3
    clock_ghz = MAX_CLOCK_GHZ
    if c.get("GRBM_GUI_ACTIVE") and rec.get("kernel_ms_profiled"):
        clock_ghz = min(MAX_CLOCK_GHZ, c["GRBM_GUI_ACTIVE"] / 8.0 / (rec["kernel_ms_profiled"] * 1e-3) / 1e9)  # held during the profiled launch
    achieved = pipe_cycles / seconds / 1e9
    peak = N_SIMDS * MAX_CLOCK_GHZ
    lane_util = c["SQ_THREAD_CYCLES_VALU"] / (c["SQ_ACTIVE_INST_VALU"] * 64.0) if c.get("SQ_ACTIVE_INST_VALU") else None
    # ... and against what this box SUSTAINS: a dense stream of independent v_fma_f32 at the kernel's waves per SIMD (measured:
    # ceilings.issue_v_fma_f32_by_waves_per_simd) at the clock the profiled launch held -- the same pipe-cycles over that rate
    of_measured = None
    if fma_by_waves and rec.get("workgroup"):
        waves = max(1.0, min(8.0, float(rec["workgroup"]) / 256.0))  # one workgroup per CU (LDS-bound): workgroup / 4 SIMDs / 64 lanes
        pts = sorted((float(w), r) for w, r in fma_by_waves.items() if r)
        rate = pts[-1][1]
        for (w0, r0), (w1, r1) in zip(pts, pts[1:]):
            if w0 <= waves <= w1:
                rate = r0 + (r1 - r0) * (waves - w0) / (w1 - w0)
        of_measured = {"value": round(achieved / (N_SIMDS * clock_ghz * cycles["f32"] * rate), 4), "waves_per_simd": waves, "v_fma_f32_per_cycle_at_that_occupancy": round(rate, 4),
                       "clock_ghz": round(clock_ghz, 3)}
    return {"achieved": round(achieved, 1), "peak": round(peak, 1), "unit": "G VALU pipe-cycles/s", "frac": round(achieved / peak, 4),
            "frac_of_measured_issue_ceiling": of_measured,
            "valu_lane_utilisation": round(lane_util, 4) if lane_util else None,
            "useful_lane_frac": round(achieved / peak * lane_util, 4) if lane_util else None,
            "valu_wave_insts_per_launch": int(valu), "f64_share": round(f64 / valu, 4), "clock_ghz_profiled": round(clock_ghz, 3),
            "issue_cycles": cycles}


def order_label(fast_scene, use_fast, verified):
    """What `--order auto` relied on, for config.order: the fast order is PROVEN bit-identical for scenes without triangles
    (rtk_optimize_info.exact == 2); with triangles it is identical in every measurement but not provable (== 1), and this run
    then stands on its own check -- both orders rendered at full size, digests compared, a mismatch fails the run."""
    if not use_fast:
        return "reference (bvh.h)"
    how = "proven bit-identical" if fast_scene.proven else ("empirically bit-identical" if fast_scene.exact else "statistical parity only")
    if fast_scene.exact and not fast_scene.proven:
        how += ", verified in this run: both orders rendered, digests equal" if verified else ", NOT verified in this run"
    return f"fast (rtk_scene_upload_fast; {how})"


def self_launch(args):
    """`python bench.py --gpus N` (N > 1, no launcher): start the N ranks ourselves.  Runs before torch is imported --
    this process never touches the GPU; it only waits for the child and forwards rank 0's JSON line."""
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
    env["RTK_BENCH_CHILD"] = "1"
    print("+ " + " ".join(cmd), file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
    return proc.wait()



def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--config", default="c2", choices=["c1", "c2", "c3", "c4", "c5"])
    p.add_argument("--width", type=int, default=0, help="override (dev only; marks the line reduced)")
    p.add_argument("--height", type=int, default=0)
    p.add_argument("--spp", type=int, default=0)
    p.add_argument("--variant", type=int, default=0, help="kernel variant (dev A/B)")
    p.add_argument("--order", default="auto", choices=["auto", "reference", "fast"],
                   help="visiting order: the reference's bvh_node order, rtk_scene_optimize's fast order, or fast where it is bit-identical (auto)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--f32", action="store_true", help="with --full: also time the f32 kernels (throughput mode, statistical parity only) and report them under f32_mode; "
                                                       "off by default: on C2 that mode is no faster than the f64 parity kernels since their box step moved to f32 culling boxes")
    p.add_argument("--no-f32", action="store_true", help="(accepted for older command lines; the f32 measurement is off unless --f32)")
    p.add_argument("--no-microbench", action="store_true", help="skip the measured ceilings (HBM copy, LDS read, VALU issue rates); nominal issue costs are used")
    p.add_argument("--no-other-order", action="store_true", help="skip the untimed render in the other visiting order (profiling runs)")
    p.add_argument("--no-other-configs", action="store_true", help="skip the short measurements of the other BASELINE configs (N = 1, default config only)")
    p.add_argument("--cpu-seconds", type=float, default=12.0, help="target duration of the CPU baseline sample")
    p.add_argument("--frames-in-flight", type=int, default=0, choices=[0, 1, 2],
                   help="2: frames alternate between two contexts and streams, so the end of one frame overlaps the start of the next; "
                        "1: one stream; 0 (default): 1 on one GPU (kernel durations in a rocprofv3 trace of this command then equal roofline.kernel_ms), 2 on several")
    p.add_argument("--sync-gather", action="store_true", help="N > 1: gather each frame before the next one is rendered (no overlap; dev A/B)")
    p.add_argument("--multi", default="ranks", choices=["ranks", "abi"],
                   help="N > 1: 'ranks' = one process per GPU, torch.distributed (RCCL) gather, the contract's launch; 'abi' = ONE process, "
                        "the product's own rtk_init_multi / rtk_render_multi_enqueue / rtk_multi_wait over N devices (what camera::render with "
                        "camera::devices does), two frames in flight.  Under the contract's launch rank 0 also runs the abi path in a child "
                        "process after its own measurement (--no-abi-path skips it) and reports it under multi_paths")
    p.add_argument("--multi-devices", default="", help="--multi abi: comma-separated HIP ordinals (default 0..N-1); an ordinal may repeat (one-GPU rehearsal)")
    p.add_argument("--no-abi-path", action="store_true")
    p.add_argument("--abi-timeout", type=float, default=150.0)
    p.add_argument("--rehearse-one-gpu", action="store_true",
                   help="dev only: run all ranks on device 0 with a gloo gather through host memory, to rehearse the N>1 control flow on a 1-GPU box")
    p.add_argument("--full", action="store_true",
                   help="also run every check and secondary measurement (pinned digest, other order, roofline, f32 mode, other configs, CPU baseline, "
                        "the abi path on N > 1); a plain run times the headline only")
    p.add_argument("--dump-outputs", default="", metavar="DIR", help="write the last timed step's outputs to DIR/<name>.npy (float32/float64, 64 MB at most)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")
    return args


def host_cores():
    """CPU cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


DUMP_LIMIT_BYTES = 64_000_000
DUMP_SAMPLE_SEED = 20260101


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: write each (name, H x W x C array, dtype) as out_dir/<name>.npy in that dtype (float32 / float64), in order,
    within `limit` bytes in all.  An array that does not fit in full is written as a fixed, seeded sample of its pixels instead:
    <name>_sample.npy (pixels x C) and <name>_sample_pixels.npy (their row-major indices, float64).  Returns the files written."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    left, written = limit, []
    for name, arr, dtype in arrays:
        arr = np.asarray(arr)
        h, w, ch = arr.shape
        item = np.dtype(dtype).itemsize
        if arr.size * item + 128 <= left:
            out = {name: arr.astype(dtype)}
        else:
            per_pixel = ch * item + 8
            k = min(h * w, max(0, (left - 256) // per_pixel))
            pixels = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(h * w, size=k, replace=False))
            out = {name + "_sample": arr.reshape(h * w, ch)[pixels].astype(dtype), name + "_sample_pixels": pixels.astype(np.float64)}
        for fname, data in out.items():
            path = os.path.join(out_dir, fname + ".npy")
            np.save(path, data)
            left -= os.path.getsize(path)
            written.append(path)
    return written


def cpu_baseline(rt, scene_name, cam, earth, target_seconds):
    """Time the CPU path on this host: reference classes if the prebuilt driver is here, else the port."""
    from oracle import orc

    cores = host_cores()
    W, H, depth = cam.image_width, cam.image_height, cam.max_depth
    if os.path.exists(orc.REF_DRIVER):
        def run(spp):
            out = subprocess.check_output([orc.REF_DRIVER, "time", scene_name, str(rt.SCENE_SEED), earth, str(W), str(H), str(spp), str(depth),
                                           str(rt.RENDER_SEED), str(cores)], timeout=600)
            return json.loads(out.decode().strip().splitlines()[-1])
        probe = run(1)
        spp = max(1, min(16, int(target_seconds / max(probe["seconds"], 1e-3))))
        res = run(spp) if spp > 1 else probe
        return {"value": round(res["msamples_per_s"], 4), "unit": "Msamples/s", "cores": cores, "kind": "reference",
                "sample": f"{scene_name} {W}x{H}x{res['spp']}spp depth {depth}, reference classes (oracle/_ref), {cores} threads, {res['seconds']:.1f} s"}
    scene = rt.Scene.build(scene_name, image_file=earth)
    def run(spp):
        c = scene.camera(W, H, spp, depth)
        t0 = time.time()
        orc.render(scene.desc_ptr, c, rt.RENDER_SEED, cores)
        return time.time() - t0
    t1 = run(1)
    spp = max(1, min(16, int(target_seconds / max(t1, 1e-3))))
    t = run(spp) if spp > 1 else t1
    return {"value": round(W * H * spp / t / 1e6, 4), "unit": "Msamples/s", "cores": cores, "kind": "port",
            "sample": f"{scene_name} {W}x{H}x{spp}spp depth {depth}, CPU restatement (oracle/rt_oracle.cpp), {cores} threads, {t:.1f} s"}


def run_abi(args):
    """--multi abi: the product's own multi-GPU path behind the C ABI, one process, N devices, two frames in flight
    (rtk_render_multi_enqueue / rtk_multi_wait, csrc/rtk_multi.cpp) -- what a sequence of camera::render calls with
    camera::devices = {0..N-1} executes.  Prints one JSON line."""
    import hashlib

    import torch

    import raytracingoneweekendapplication_amd as rt

    devices = [int(x) for x in args.multi_devices.split(",")] if args.multi_devices else list(range(args.gpus))
    n = len(devices)
    scene_name = rt.CONFIG_SCENES[args.config]
    tmp = tempfile.mkdtemp(prefix="rtk_bench_")
    earth = rt.write_synthetic_earth(os.path.join(tmp, "earth_synth.ppm"))
    scene = rt.Scene.build(scene_name, rt.SCENE_SEED, earth)
    cam = scene.camera(args.width, args.height, args.spp, 0)
    W, H, spp = cam.image_width, cam.image_height, cam.samples_per_pixel
    fast_scene = scene.fast_order(cam.center)
    use_fast = args.order == "fast" or (args.order == "auto" and fast_scene.exact)
    multi = rt.MultiRenderer(devices)
    multi.upload_fast(scene, cam.center) if use_fast else multi.upload(scene)
    dev = torch.device("cuda", devices[0])
    torch.cuda.set_device(dev)
    images = [torch.empty((H, W, 3), dtype=torch.float64, device=dev) for _ in range(2)]
    rgb8s = [torch.empty((H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2)]

    def sync_all():
        for d in sorted(set(devices)):
            torch.cuda.synchronize(d)

    for k in range(max(args.warmup, 1)):  # every context learns its tile hand-out order from an untimed frame
        multi.enqueue_device(cam, images[k % 2].data_ptr(), rgb8s[k % 2].data_ptr(), variant=args.variant)
    multi.wait()
    sync_all()
    t0 = time.perf_counter()
    for k in range(args.steps):
        multi.enqueue_device(cam, images[k % 2].data_ptr(), rgb8s[k % 2].data_ptr(), variant=args.variant)
    multi.wait()
    sync_all()
    elapsed = time.perf_counter() - t0
    last = images[(args.steps - 1) % 2]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, [("image", last.cpu().numpy(), "float64"), ("rgb8", rgb8s[(args.steps - 1) % 2].cpu().numpy(), "float32")])
    checksum = hashlib.sha256(last.cpu().numpy().tobytes()).hexdigest()[:16]
    t0 = time.perf_counter()
    for k in range(args.steps):  # the blocking form: what a single camera::render() call costs per frame
        multi.render_device(cam, images[0].data_ptr(), rgb8s[0].data_ptr(), variant=args.variant)
    sync_all()
    blocking = time.perf_counter() - t0
    samples = W * H * spp
    line = {"metric": "Msamples/sec (pixels x spp) on RTIOW final scene 1920x1080", "value": round(samples * args.steps / elapsed / 1e6, 2), "unit": "Msamples/s",
            "n_gpus": n, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{scene_name} {W}x{H}x{spp}spp depth {cam.max_depth} (BASELINE configs[{int(args.config[1]) - 1}])" + WORKLOAD_NOTES.get(args.config, ""),
                       "parallelism": f"one process, rtk_render_multi_enqueue over devices {devices}: interleaved 8x8 tiles, one gather per frame "
                                      f"({'ncclGather (RCCL)' if multi.uses_rccl else 'peer copies'}), two frames in flight",
                       "order": order_label(fast_scene, use_fast, False), "reduced": bool(args.width or args.height or args.spp), "variant": args.variant},
            "multi": "abi", "uses_rccl": multi.uses_rccl, "devices": devices,
            "blocking_render_multi": {"value": round(samples * args.steps / blocking / 1e6, 2), "unit": "Msamples/s", "ms_per_step": round(blocking / args.steps * 1e3, 4),
                                      "note": "rtk_render_multi_device per frame: enqueue + wait, no overlap between frames"},
            "framebuffer_sha256": checksum}
    print(json.dumps(line), flush=True)
    multi.close()


def abi_path_in_child(args, timeout_s):
    """Rank 0 of the contract's launch: time the product's own multi-GPU path (--multi abi) over the same N devices in a child
    process while the ranks idle.  Reported, never required: a failure or a timeout becomes an `error` string."""
    cmd = [sys.executable, os.path.abspath(__file__), "--multi", "abi", "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(max(args.warmup, 1)),
           "--config", args.config, "--order", args.order]
    for flag, val in (("--width", args.width), ("--height", args.height), ("--spp", args.spp), ("--variant", args.variant)):
        if val:
            cmd += [flag, str(val)]
    if args.rehearse_one_gpu:  # every rank of the rehearsal shares device 0: so do the child's device slots
        cmd += ["--multi-devices", ",".join(["0"] * args.gpus)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RTK_BENCH_CHILD",
                                                              "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "TORCHELASTIC_RUN_ID")}
    try:
        proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        try:
            out, err = proc.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            proc.kill()
            proc.communicate()
            return {"error": f"timed out after {timeout_s:.0f} s"}
        if proc.returncode != 0:
            return {"error": f"exit code {proc.returncode}: {err.strip().splitlines()[-1] if err.strip() else ''}"[:300]}
        return json.loads(out.strip().splitlines()[-1])
    except Exception as exc:
        return {"error": str(exc)[:300]}


def main():
    args = parse_args()
    if args.multi == "abi":
        return run_abi(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    if os.environ.get("RTK_BENCH_LAUNCH_ONLY"):  # tests of the launcher on boxes without a GPU: report the rank environment, touch nothing
        sys.stdout.write(json.dumps({"launch_only": True, "rank": int(os.environ.get("RANK", "0")), "world": int(os.environ.get("WORLD_SIZE", "1")),
                                     "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "gpus": args.gpus, "master": os.environ.get("MASTER_ADDR")}) + "\n")
        sys.stdout.flush()  # one write per line: the ranks share the parent's pipe
        return
    import torch
    import torch.distributed as dist

    import raytracingoneweekendapplication_amd as rt
    from raytracingoneweekendapplication_amd import tiling

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n = args.gpus
    if world != n:  # under a launcher the launcher's world size is the truth
        n = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU path exists for the product)")
    if args.rehearse_one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if n > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.rehearse_one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=n)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=n, device_id=dev)

    # ---- inputs: scene + camera, resident in HBM before anything is timed
    scene_name = rt.CONFIG_SCENES[args.config]
    tmp = tempfile.mkdtemp(prefix="rtk_bench_")
    earth = rt.write_synthetic_earth(os.path.join(tmp, "earth_synth.ppm"))
    scene = rt.Scene.build(scene_name, rt.SCENE_SEED, earth)
    cam = scene.camera(args.width, args.height, args.spp, 0)
    W, H, spp, depth = cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth
    reduced = bool(args.width or args.height or args.spp)
    fast_scene = scene.fast_order(cam.center)
    use_fast = args.order == "fast" or (args.order == "auto" and fast_scene.exact)
    with_other_order = args.full and not args.no_other_order
    order_name = order_label(fast_scene, use_fast, with_other_order)
    renderer = rt.Renderer(local_rank)
    other_renderer = rt.Renderer(local_rank) if with_other_order else None
    for r_, fast_ in ((renderer, use_fast), (other_renderer, not use_fast)):
        if r_ is None:
            continue
        if fast_:
            r_.upload_fast(scene, cam.center)   # rtk_scene_optimize + upload, fused slab test on the grown boxes
        else:
            r_.upload(scene)                    # the reference's own hierarchy and order
    info = renderer.scene_info()
    stream = torch.cuda.current_stream().cuda_stream

    # Two frames in flight: frames alternate between two contexts (own workspace, work counter and learned tile order)
    # on two streams, so that the drain of frame k -- a few long paths on otherwise idle CUs -- overlaps the start of
    # frame k+1 (measured at kernel level: +1 % at N = 1, +6 % on an eighth of the frame; tools/overlap_probe.py).
    if args.frames_in_flight == 0:
        args.frames_in_flight = 1 if n == 1 else 2
    main_renderers = [renderer]
    if args.frames_in_flight == 2:
        second = rt.Renderer(local_rank)
        second.upload_fast(scene, cam.center) if use_fast else second.upload(scene)
        main_renderers.append(second)
    side_stream = torch.cuda.Stream(dev) if args.frames_in_flight == 2 else None

    def make_step(real_mode, renderers):
        dtype = torch.float64 if real_mode == rt.RTK_REAL_F64 else torch.float32
        tpr = tiling.tiles_per_rank(W, H, n)
        slots = len(renderers)
        streams = [torch.cuda.current_stream(), side_stream][:slots]
        images = [torch.empty((H, W, 3), dtype=dtype, device=dev) if rank == 0 else None for _ in range(slots)]
        rgb8s = [torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if rank == 0 else None for _ in range(slots)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        state = {"frame": 0}

        def unpermute(gathered, slot):  # rank 0: [n, tiles_per_rank, 3, 64] -> the row-major image + bytes
            i = slot % slots
            if gathered.device != dev:  # gloo rehearsal: the gather went through host memory
                gathered = gathered.to(dev)
            renderers[i].unpermute(W, H, n, real_mode, gathered.data_ptr(), images[i].data_ptr(), rgb8s[i].data_ptr(), stream=streams[i].cuda_stream)

        # N > 1: two compact tile buffers per rank; the gather of frame k runs while frame k+1 renders (tiling.GatherPipeline)
        pipe = None
        if n > 1 and not args.sync_gather:
            pipe = tiling.GatherPipeline(n, rank, lambda: torch.empty((tpr, 3, 64), dtype=dtype, device=dev), unpermute, stage_to_host=args.rehearse_one_gpu,
                                         streams=streams if slots == 2 else None)
        compact = torch.empty((tpr, 3, 64), dtype=dtype, device=dev) if (n > 1 and pipe is None) else None

        def step(kernel_ms=None):
            i = state["frame"] % slots
            state["frame"] += 1
            r, st = renderers[i], streams[i]
            if kernel_ms is not None:
                ev[0].record(st)
            if n == 1:
                r.render_device(cam, images[i].data_ptr(), rgb8s[i].data_ptr(), real_mode=real_mode, variant=args.variant, stream=st.cuda_stream)
            else:
                target = pipe.next_buffer() if pipe is not None else compact
                r.render_device(cam, target.data_ptr(), 0, real_mode=real_mode, rank=rank, n_ranks=n, variant=args.variant, stream=st.cuda_stream)
            if kernel_ms is not None:
                ev[1].record(st)
            if pipe is not None:
                pipe.submit()  # starts this frame's gather, completes the previous frame (gather wait + un-permute on rank 0)
            elif n > 1:
                with torch.cuda.stream(st):
                    if args.rehearse_one_gpu:  # gloo has no device gather: stage through host memory (rehearsal only)
                        gathered = tiling.gather_to_root(compact.cpu(), n, rank)
                    else:
                        gathered = tiling.gather_to_root(compact, n, rank)
                    if rank == 0:
                        unpermute(gathered, i)
            if kernel_ms is not None:
                ev[1].synchronize()
                kernel_ms.append(ev[0].elapsed_time(ev[1]))

        def flush():  # completes the frame still in flight; part of the timed region
            if pipe is not None:
                pipe.flush()

        def last_outputs():  # what the last step handed its caller (rank 0): the linear image and its 8-bit bytes
            i = (state["frame"] - 1) % slots
            return images[i], rgb8s[i]
        return step, flush, last_outputs, slots

    def barrier():
        if n > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(real_mode, steps, warmup, renderers=None, kernel_time=True, keep_outputs=False):
        step, flush, last_outputs, slots = make_step(real_mode, renderers or main_renderers)
        if warmup > 0:
            for _ in range(max(0, slots - warmup)):  # every context needs one untimed frame to learn its tile order
                step()
        for _ in range(warmup):
            step()
        flush()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        flush()
        barrier()
        elapsed = time.perf_counter() - t0
        if n > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        # the last timed step's outputs, copied to the host before anything else runs on them
        outputs = [t.cpu().numpy() for t in last_outputs()] if keep_outputs and rank == 0 else None
        if not kernel_time:
            return elapsed, None, last_outputs()[0], outputs
        # kernel duration: separate, event-bracketed launches on the same stream (not inside the timed region)
        kernel_ms = []
        for _ in range(min(steps, 5)):
            step(kernel_ms)
        flush()
        barrier()
        return elapsed, sum(kernel_ms) / len(kernel_ms), last_outputs()[0], outputs

    import hashlib

    # a plain run times the headline only; the per-launch kernel time (roofline, other order) is measured with --full
    elapsed, kernel_ms, image, outputs = timed(rt.RTK_REAL_F64, args.steps, args.warmup, kernel_time=args.full, keep_outputs=bool(args.dump_outputs))
    if outputs is not None:
        dump_outputs(args.dump_outputs, [("image", outputs[0], "float64"), ("rgb8", outputs[1], "float32")])
    checksum = None
    if rank == 0 and args.full:  # a digest of the framebuffer: must not depend on the number of GPUs
        checksum = hashlib.sha256(image.cpu().numpy().tobytes()).hexdigest()[:16]
    if rank == 0 and args.full and not reduced and checksum != PINNED_SHA256.get(args.config, checksum):  # the same frame on any GPU count, in any round
        raise SystemExit(f"{args.config}: framebuffer digest {checksum} differs from the pinned one {PINNED_SHA256[args.config]}")
    samples_per_step = W * H * spp
    value = samples_per_step * args.steps / elapsed / 1e6

    # ---- the other visiting order, outside the timed region: its rate, and the proof that both orders give the same bytes
    other_steps = max(1, min(args.steps, 3))
    other = None
    if with_other_order:
        o_elapsed, o_kernel_ms, o_image, _ = timed(rt.RTK_REAL_F64, other_steps, 1, [other_renderer])
    if rank == 0 and with_other_order:
        o_sum = hashlib.sha256(o_image.cpu().numpy().tobytes()).hexdigest()[:16]
        other = {"order": "reference (bvh.h)" if use_fast else "fast (rtk_scene_upload_fast)", "value": round(samples_per_step * other_steps / o_elapsed / 1e6, 2),
                 "unit": "Msamples/s", "kernel_ms": round(o_kernel_ms, 4), "framebuffer_sha256": o_sum, "identical_framebuffer": o_sum == checksum,
                 "fast_order_exact": fast_scene.exact, "fast_order_info": fast_scene.info}
        if fast_scene.exact and o_sum != checksum:
            raise SystemExit(f"fast order claims bit-identity but the framebuffers differ: {checksum} vs {o_sum}")
    if with_other_order:
        del o_image

    # ---- roofline of the render kernel on rank 0.  Bound: VALU issue (see the module docstring); the HBM byte model of
    # SURVEY 8(d) and the PMC-measured HBM traffic are reported beside it.
    roofline = None
    counters = None
    workload = f"{scene_name} {W}x{H}x{spp}"
    if rank == 0 and args.full:
        d_cnt = torch.zeros(12, dtype=torch.int64, device=dev)
        tpr = tiling.tiles_per_rank(W, H, n)
        scratch = torch.empty((tpr * 192,), dtype=torch.float64, device=dev) if n > 1 else torch.empty((H, W, 3), dtype=torch.float64, device=dev)
        # the counting instantiation of the kernel that was timed (same program, same steps) -- exact integers
        renderer.render_device(cam, scratch.data_ptr(), 0, real_mode=rt.RTK_REAL_F64, rank=rank, n_ranks=n, d_counters=d_cnt.data_ptr(), variant=args.variant, stream=stream)
        torch.cuda.synchronize()
        counters = dict(zip(rt.COUNTER_FIELDS, [int(v) for v in d_cnt.tolist()]))
        kernel = renderer.kernel_name(rt.RTK_REAL_F64, args.variant)
        mixed = ", 256u," in kernel  # F_F32_BOX: 32-byte f32 culling-box records
        b_sample = rt.algorithmic_bytes_per_sample(counters, spp, rt.RTK_REAL_F64, f32_boxes=mixed)
        bytes_per_launch = b_sample * counters["samples"]
        model_gbs = bytes_per_launch / (kernel_ms * 1e-3) / 1e9
        hbm_model = {"algorithmic_bytes_per_sample": round(b_sample, 2), "algorithmic_bytes_per_launch": int(bytes_per_launch),
                     "model_GBps": round(model_gbs, 1), "hbm_peak_GBps": HBM_PEAK_GBS, "compulsory_bytes": info["bytes_f64"] + W * H * 3 * 9,
                     "box_record_bytes": 32 if mixed else 56,
                     "note": "SURVEY 8(d) byte model x exact work counters of the timed kernel's counting build / kernel time.  A model of bytes "
                             "touched, NOT HBM traffic and not a roofline fraction: the traversal program is staged in LDS, so model_GBps may exceed hbm_peak_GBps",
                     "per_sample": {k: round(counters[k] / counters["samples"], 4) for k in rt.COUNTER_FIELDS if k != "samples"}}
        rec, why = (None, "reduced workload: PMC profiles exist for the full-size configs only") if reduced or args.variant else load_pmc(args.config, kernel, workload, n)
        roofline = {"bound": "valu", "achieved": None, "peak": round(N_SIMDS * MAX_CLOCK_GHZ, 1), "unit": "G VALU pipe-cycles/s", "frac": None, "traffic": None,
                    "kernel": kernel, "kernel_ms": round(kernel_ms, 4),
                    # a frame with more than 21 sample chunks (spp > 168) is several launches of the kernel; kernel_ms and every counter are per FRAME
                    "launches_per_frame": rt.hip_lib().rtk_frame_launches(ctypes.byref(cam), ctypes.byref(rt.RenderOpts(rt.RENDER_SEED, rt.RTK_REAL_F64, rank, n, 0, args.variant, None)))}
        # measured ceilings of THIS box (csrc/rtk_microbench.hip): achievable HBM rate from a stream copy, the LDS
        # read rate the byte model is served at, and the issue cost of each VALU class the roofline prices
        measured, measured_why = None, None
        if not args.no_microbench:
            try:
                measured = rt.microbench(local_rank)
            except Exception as exc:  # a measurement tool: its absence degrades the line (nominal costs), never the run
                measured_why = str(exc)[:200]
        cycles, cycles_source = issue_cycles(measured)
        roofline["ceilings"] = {"source": "csrc/rtk_microbench.hip, this run" if measured else f"unavailable: {measured_why}",
                                "hbm_spec_GBps": HBM_PEAK_GBS,
                                "hbm_copy_GBps": round(measured["hbm_copy_GBps"], 1) if measured else None,
                                "hbm_read_GBps": round(measured["hbm_read_GBps"], 1) if measured else None,
                                "lds_read_b128_GBps": round(measured["lds_read_b128_GBps"], 1) if measured else None,
                                "lds_read_b128_random_records_GBps": round(measured["lds_read_b128_random_GBps"], 1) if measured else None,
                                "lds_roundtrip_cycles": round(measured["lds_roundtrip_cycles"], 1) if measured else None,
                                "shader_clock_GHz_under_valu_load": round(measured.get("clock_dense_valu_GHz") or measured["shader_clock_GHz"], 3) if measured else None,
                                "issue_v_fma_f32_by_waves_per_simd": ({w: round(measured[k], 4) for w, k in (("1", "issue_v_fma_f32_1wave"), ("2", "issue_v_fma_f32_2waves"),
                                                                                                               ("4", "issue_v_fma_f32_4waves"), ("8", "issue_v_fma_f32_8waves")) if measured.get(k)}
                                                                      if measured else None),
                                # DVFS (MI355X_MICROARCH.md): the in-kernel clock, s_memtime / s_memrealtime x 100 MHz, with every SIMD issuing
                                # v_fma_f32 from 8 waves after 0.3 s of back-to-back launches, and on a nearly idle chip (one wave per CU)
                                "clock_dense_valu_GHz": round(measured["clock_dense_valu_GHz"], 3) if measured and measured.get("clock_dense_valu_GHz") else None,
                                "clock_light_load_GHz": round(measured["clock_light_load_GHz"], 3) if measured and measured.get("clock_light_load_GHz") else None,
                                "issue_cycles_per_wave_instruction": cycles, "issue_cycles_source": cycles_source,
                                "issue_rates_measured": {k: round(v, 4) for k, v in measured.items() if k.startswith("issue_")} if measured else None}
        if measured:
            lds_rate = measured["lds_read_b128_GBps"]
            hbm_model["model_vs_lds_ceiling"] = round(model_gbs / lds_rate, 4) if lds_rate > 0 else None
            hbm_model["lds_ceiling_GBps"] = round(lds_rate, 1)
            hbm_model["lds_random_record_probe_GBps"] = round(measured["lds_read_b128_random_GBps"], 1)
            hbm_model["note"] += ("; model_vs_lds_ceiling = model_GBps / the measured conflict-free ds_read_b128 rate of the chip (every lane its own 16 bytes); "
                                  "lds_random_record_probe_GBps = a probe reading per-lane random 32-byte records behind an address computation of its own "
                                  "(bank conflicts included) -- a lower bound of the random-record rate, not a ceiling")
        # the work-based fraction: exact work counters x ISA-derived cost per unit of work (lean MIXED kernel family)
        isa, isa_why = load_isa_costs()
        if isa is not None and mixed:
            roofline.update(work_roofline(counters, isa, cycles, kernel_ms))
            roofline["work_frac_source"] = {"isa_costs": isa_why, "issue_cycles": cycles_source, "counters": "counting build of the timed kernel, this run"}
        else:
            roofline["work_frac"] = None
            roofline["work_frac_source"] = {"refused": isa_why if isa is None else "ISA cost table covers the lean MIXED kernel family only"}
        if rec is not None:
            roofline.update(valu_roofline(rec, kernel_ms, cycles, roofline["ceilings"].get("issue_v_fma_f32_by_waves_per_simd")))
            roofline["traffic"] = rec.get("hbm_bytes_per_launch")
            roofline["hbm_traffic_GBps"] = round(rec["hbm_bytes_per_launch"] / (kernel_ms * 1e-3) / 1e9, 1) if rec.get("hbm_bytes_per_launch") else None
            roofline["hbm_frac_of_peak"] = round(roofline["hbm_traffic_GBps"] / HBM_PEAK_GBS, 5) if roofline["hbm_traffic_GBps"] else None
            roofline["pmc"] = {"source": why, "source_hash": rec["source_hash"], "kernel_ms_profiled": rec.get("kernel_ms_profiled"),
                               "wait_share": rec.get("wait_share"), "lds_bank_conflict_share": rec.get("lds_bank_conflict_share"),
                               "vgpr": rec.get("vgpr"), "scratch_bytes_per_lane": rec.get("scratch")}
        else:
            roofline["pmc"] = {"source": None, "refused": why}
        roofline["hbm_model"] = hbm_model
        roofline["note"] = ("frac = VALU pipe-cycles consumed (PMC wave-instruction counts x the issue cycles of their class, ceilings.issue_cycles_per_wave_instruction) "
                            "/ (1024 SIMDs x 2.4 GHz x kernel time): a utilisation of what was executed, against the SPEC rate (one v_fma_f32 per 2 cycles at 2.4 GHz); "
                            "frac_of_measured_issue_ceiling = the same pipe-cycles against what a dense stream of independent v_fma_f32 sustains on this box at the "
                            "kernel's waves per SIMD and at the clock the profiled launch held; useful_lane_frac = frac x VALU lane utilisation.  "
                            "work_frac = (exact work counters x ISA-derived instruction cost per unit of work / 64 lanes) / the same denominator: what the frame's "
                            "necessary arithmetic would occupy on full waves -- it cannot rise by executing more instructions.  kernel_ms: HIP events on the "
                            "launch stream, one launch alone on the device")

    f32_mode = None
    if args.full and args.f32 and not args.no_f32:
        e32, k32, _, _ = timed(rt.RTK_REAL_F32, max(1, min(args.steps, 3)), 1)
        if rank == 0:
            f32_mode = {"value": round(samples_per_step * max(1, min(args.steps, 3)) / e32 / 1e6, 2), "unit": "Msamples/s", "kernel_ms": round(k32, 4),
                        "note": "throughput mode; parity vs the double reference is statistical only (SURVEY.md 8(d)); not the headline"}

    # ---- the other BASELINE configs (parity-test cases, not the headline): a few frames each at full size, in the order and
    # with the kernel `--config cN` would time, so that their rates are on the driver's record too.  N = 1, default config only.
    other_configs = None
    if args.full and rank == 0 and n == 1 and args.config == "c2" and not reduced and not args.variant and not args.no_other_configs:
        other_configs = {}
        for cfg in ("c3", "c4", "c5"):
            # A failure here fails the run: an exception propagates, and a fast order that claims bit-identity is checked
            # against the reference order at full size (one frame of the other order, digests compared) like the headline is.
            name_ = rt.CONFIG_SCENES[cfg]
            scene_ = rt.Scene.build(name_, rt.SCENE_SEED, earth)
            cam_ = scene_.camera(0, 0, 0, 0)
            fast_ = scene_.fast_order(cam_.center)
            r_, r2_ = rt.Renderer(local_rank), rt.Renderer(local_rank)
            for rr_, f_ in ((r_, fast_.exact), (r2_, not fast_.exact)):
                rr_.upload_fast(scene_, cam_.center) if f_ else rr_.upload(scene_)
            W_, H_, spp_ = cam_.image_width, cam_.image_height, cam_.samples_per_pixel
            img_ = torch.empty((H_, W_, 3), dtype=torch.float64, device=dev)
            u8_ = torch.empty((H_, W_, 3), dtype=torch.uint8, device=dev)
            frames = 2 if cfg == "c5" else 3
            r_.render_device(cam_, img_.data_ptr(), u8_.data_ptr(), real_mode=rt.RTK_REAL_F64, stream=stream)  # untimed: learns the tile order
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                r_.render_device(cam_, img_.data_ptr(), u8_.data_ptr(), real_mode=rt.RTK_REAL_F64, stream=stream)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            sha_ = hashlib.sha256(img_.cpu().numpy().tobytes()).hexdigest()[:16]
            sha8_ = hashlib.sha256(u8_.cpu().numpy().tobytes()).hexdigest()[:16]
            t0 = time.perf_counter()
            r2_.render_device(cam_, img_.data_ptr(), u8_.data_ptr(), real_mode=rt.RTK_REAL_F64, stream=stream)
            torch.cuda.synchronize()
            dt2 = time.perf_counter() - t0
            sha2_ = hashlib.sha256(img_.cpu().numpy().tobytes()).hexdigest()[:16]
            other_configs[cfg] = {"workload": f"{name_} {W_}x{H_}x{spp_}spp depth {cam_.max_depth}" + WORKLOAD_NOTES.get(cfg, ""),
                                  "value": round(W_ * H_ * spp_ * frames / dt / 1e6, 2), "unit": "Msamples/s", "ms_per_step": round(dt / frames * 1e3, 3),
                                  "steps": frames, "dtype": "f64", "order": order_label(fast_, fast_.exact, True),
                                  "kernel": r_.kernel_name(rt.RTK_REAL_F64, 0), "framebuffer_sha256": sha_, "rgb8_sha256": sha8_,
                                  "other_order": {"order": "reference (bvh.h)" if fast_.exact else "fast (rtk_scene_upload_fast)", "framebuffer_sha256": sha2_,
                                                  "value": round(W_ * H_ * spp_ / dt2 / 1e6, 2), "steps": 1, "identical_framebuffer": sha2_ == sha_}}
            if fast_.exact and sha2_ != sha_:
                raise SystemExit(f"{cfg}: the fast order claims bit-identity but the framebuffers differ: {sha_} vs {sha2_}")
            if cfg in PINNED_SHA256 and not reduced and sha_ != PINNED_SHA256[cfg]:
                raise SystemExit(f"{cfg}: framebuffer digest {sha_} differs from the pinned one {PINNED_SHA256[cfg]} (tests/test_gpu_parity.py pins the same values)")
            del r_, r2_, img_, u8_, scene_

    cpu = None
    if args.full and rank == 0 and n == 1 and not args.no_cpu_baseline:
        try:
            cpu = cpu_baseline(rt, scene_name, cam, earth, args.cpu_seconds)
        except Exception as exc:  # the baseline is reported, never required
            cpu = {"value": None, "unit": "Msamples/s", "cores": host_cores(), "kind": "unavailable", "sample": f"failed: {exc}"}

    # ---- N > 1: the product's own multi-GPU path (rtk_render_multi_enqueue behind the C ABI: one process, N devices) beside the
    # torch.distributed ranks that were just timed -- in a child process of rank 0, while every rank idles at a CPU barrier
    multi_paths = None
    if args.full and n > 1 and not args.no_abi_path:
        idle = dist.new_group(backend="gloo")
        torch.cuda.synchronize()
        dist.barrier(group=idle)
        abi = abi_path_in_child(args, args.abi_timeout) if rank == 0 else None
        dist.barrier(group=idle)
        if rank == 0:
            multi_paths = {"ranks": {"value": round(value, 2), "unit": "Msamples/s", "what": "one process per GPU, torch.distributed (RCCL) gather, two frames in flight: the value of this line"},
                           "abi": ({k: abi.get(k) for k in ("value", "unit", "ms_per_step", "uses_rccl", "devices", "blocking_render_multi", "framebuffer_sha256", "error") if k in abi}
                                   | {"what": "one process, rtk_render_multi_enqueue / rtk_multi_wait over the same devices (csrc/rtk_multi.cpp), two frames in flight"}),
                           "identical_framebuffer": (abi.get("framebuffer_sha256") == checksum) if "framebuffer_sha256" in abi else None}
    if rank == 0:
        line = {
            "metric": "Msamples/sec (pixels x spp) on RTIOW final scene 1920x1080",
            "value": round(value, 2), "unit": "Msamples/s", "n_gpus": n, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{scene_name} {W}x{H}x{spp}spp depth {depth} (BASELINE configs[{int(args.config[1]) - 1}])" + WORKLOAD_NOTES.get(args.config, ""),
                       "tiles": "8x8 px per wave, interleaved over ranks", "parallelism": (f"image tiles over {n} GPU(s) + 1 gather per frame" + ("" if args.sync_gather else ", overlapped with the next frame")) if n > 1 else "1 GPU",
                       "scene_seed": rt.SCENE_SEED, "render_seed": rt.RENDER_SEED, "program_ops": info["program_ops"], "reduced": reduced,
                       "variant": args.variant, "order": order_name, "frames_in_flight": args.frames_in_flight},
            "roofline": roofline,
            "cpu_baseline": cpu,
            "f32_mode": f32_mode,
            "other_order": other,
            "other_configs": other_configs,
            "multi_paths": multi_paths,
            "speedup_vs_cpu_baseline": (round(value / cpu["value"], 1) if cpu and cpu.get("value") else None),
            "framebuffer_sha256": checksum,
        }
        print(json.dumps(line), flush=True)
    if n > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
