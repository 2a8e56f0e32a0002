"""What a set of small frames costs as one view batch (rtk_render_views), beside the two routes a caller had before: a loop of
rtk_render_device over the same cameras, and rtk_query_radiance over the same cameras' rays on resident records.

Scenes: book1_final and cornell_box, fast order, f64 and f32, 16 samples per pixel at the scene's depth.  Shapes:
  6 x 256x256     a cube capture (rt.cube_face_cameras at the scene camera's position)
  64 x 64x64      an orbit of the scene's camera
  256 x 32x32     the same orbit, finer
  1 x 1920x1080   one full frame: the price of the per-lane camera reads against the plain kernel
For each scene, mode and shape
  batch   rtk_render_views into [N][H][W][3]
  loop    rtk_render_device per camera into the same planes (the plain kernels: their code is the parent commit's, tools/isa_diff.py)
  query   rtk_query_radiance with samples = 1 over the N x H x W x 16 records that rtk_lens_rays wrote for the cameras (resident;
          writing them and the per-pixel sum the caller would still owe are not timed)
are timed with device events: a warm-up, then the median of --reps runs -- in each of --processes fresh processes, one after the
other (never two with the GPU open).  Reported: the median over the processes and max - min over them.  The first process also
checks that batch and loop wrote the same bits.
What the protocol does not control: a timed window holds the host's enqueue work as far as the device had to wait for it (a
loop of N frames is N x 4 enqueues); the three routes of a shape run one after the other; differences inside the reported
spread are not resolved by it.

    python tools/view_batch_probe.py [--json profiles/view_batch_probe.json] [--processes 3] [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPP, SEED = 16, 1
SCENES = ("book1_final", "cornell_box")
SHAPES = (("cube", 6, 256, 256), ("orbit", 64, 64, 64), ("orbit", 256, 32, 32), ("frame", 1, 1920, 1080))
RAY_BYTES = 88


def orbit(rt, cam, angle):
    """`cam` turned by `angle` about the vertical axis through the point three viewport distances ahead of it."""
    out = rt.Camera.from_buffer_copy(cam)
    vec = lambda v: (v.x, v.y, v.z)  # noqa: E731
    c, p00, du, dv = vec(cam.center), vec(cam.pixel00_loc), vec(cam.pixel_delta_u), vec(cam.pixel_delta_v)
    mid = [p00[k] + du[k] * (cam.image_width - 1) / 2 + dv[k] * (cam.image_height - 1) / 2 for k in range(3)]
    pivot = [c[k] + 3.0 * (mid[k] - c[k]) for k in range(3)]
    cs, sn = math.cos(angle), math.sin(angle)
    turn = lambda v: (cs * v[0] + sn * v[2], v[1], -sn * v[0] + cs * v[2])  # noqa: E731
    about = lambda p: tuple(pivot[k] + t for k, t in enumerate(turn([p[k] - pivot[k] for k in range(3)])))  # noqa: E731
    out.center, out.pixel00_loc = rt.Vec3(*about(c)), rt.Vec3(*about(p00))
    out.pixel_delta_u, out.pixel_delta_v = rt.Vec3(*turn(du)), rt.Vec3(*turn(dv))
    out.defocus_disk_u, out.defocus_disk_v = rt.Vec3(*turn(vec(cam.defocus_disk_u))), rt.Vec3(*turn(vec(cam.defocus_disk_v)))
    return out


def worker(args) -> None:
    import torch

    import raytracingoneweekendapplication_amd as rt

    r = rt.Renderer(0)
    earth = rt.write_synthetic_earth(os.path.join(tempfile.mkdtemp(), "earth_synth.ppm"))
    rows = []

    def timed(fn):
        times = []
        for rep in range(args.reps + 1):                          # rep 0: warm-up
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(t0.elapsed_time(t1))
        return statistics.median(times)

    for name in SCENES:
        scene = rt.Scene.build(name, rt.SCENE_SEED, earth)
        full = scene.camera(1920, 1080, SPP, 0)
        depth, bg = full.max_depth, (full.background.x, full.background.y, full.background.z)
        r.upload_fast(scene, full.center)
        for real_mode, dt, label in ((rt.RTK_REAL_F64, torch.float64, "f64"), (rt.RTK_REAL_F32, torch.float32, "f32")):
            for kind, n, w, h in SHAPES:
                base = scene.camera(w, h, SPP, 0)
                if kind == "cube":
                    cams = rt.cube_face_cameras((full.center.x, full.center.y, full.center.z), w, spp=SPP, max_depth=depth, background=bg)
                else:
                    cams = [orbit(rt, base, 2.0 * math.pi * v / n) for v in range(n)]
                px = w * h
                d_batch = torch.zeros((n, px, 3), dtype=dt, device="cuda")
                d_loop = torch.zeros((n, px, 3), dtype=dt, device="cuda")
                d_rays = torch.zeros(n * px * SPP * RAY_BYTES, dtype=torch.uint8, device="cuda")
                d_rad = torch.zeros((n * px * SPP, 3), dtype=dt, device="cuda")
                kw = dict(seed=SEED, real_mode=real_mode)
                plane = px * 3 * d_loop.element_size()
                for v, cam in enumerate(cams):
                    r.lens_rays_device(rt.derive_lens(cam=cam), SPP, d_rays.data_ptr() + v * px * SPP * RAY_BYTES, **kw)

                def loop():
                    for v, cam in enumerate(cams):
                        r.render_device(cam, d_loop.data_ptr() + v * plane, **kw)

                row = {"what": "batch against loop and query", "scene": name, "real": label, "views": n, "width": w, "height": h, "spp": SPP, "depth": depth,
                       "kernel": r.view_kernel_name(real_mode),
                       "batch_ms": round(timed(lambda: r.render_views_device(cams, d_batch.data_ptr(), **kw)), 4),
                       "loop_ms": round(timed(loop), 4),
                       "query_ms": round(timed(lambda: r.query_radiance_device(n * px * SPP, d_rays.data_ptr(), d_rad.data_ptr(), max_depth=depth, background=bg,
                                                                                samples=1, **kw)), 4)}
                if args.first:
                    row["identical"] = bool(torch.equal(d_batch, d_loop))
                rows.append(row)
                print(row, flush=True)
                del d_batch, d_loop, d_rays, d_rad
    r.close()
    with open(args.worker, "w") as f:
        json.dump(rows, f)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "view_batch_probe.json"))
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--first", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return
    tmp = tempfile.mkdtemp()
    runs = []
    for p in range(args.processes):                               # fresh processes, one after the other
        path = os.path.join(tmp, f"run{p}.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", path, "--reps", str(args.reps)] + (["--first"] if p == 0 else [])
        subprocess.run(cmd, check=True, timeout=900)
        runs.append(json.load(open(path)))
    rows = []
    key = lambda row: (row["scene"], row["real"], row["views"], row["width"])  # noqa: E731
    for first in runs[0]:
        same = [row for run in runs for row in run if key(row) == key(first)]
        row = dict(first, processes=len(same))
        for field in [f for f in first if f.endswith("_ms")]:
            values = [s[field] for s in same]
            row[field] = round(statistics.median(values), 4)
            row[field.replace("_ms", "_spread_ms")] = round(max(values) - min(values), 4)
        row["loop_over_batch"] = round(row["loop_ms"] / row["batch_ms"], 3)
        row["query_over_batch"] = round(row["query_ms"] / row["batch_ms"], 3)
        rows.append(row)
        print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
