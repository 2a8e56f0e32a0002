"""What temporal accumulation costs and what it buys (rtk_temporal_accumulate).

Times, on C3 (cornell_box) in the fast order, f64 and f32, at 1920x1080 and 800x800, in one run: the temporal pass (the camera
turns one degree around the room between calls, back and forth, so every call reprojects; outputs: colour, se, bytes and history
length), ONE iteration of the guided filter (rtk_denoise_guided, iterations = 1) and the 4-sample guide pass -- device events
around synchronised work, one warm-up, --reps timed runs, the median.  Then the quality numbers of tests/test_temporal.py: 8
frames of 16 spp along that orbit at 200x200, and after every frame the mean squared error of the accumulated image and of the
frame alone against a 1024-spp frame of another seed at the same camera, before and after the guided filter.  Prints one line per
row; --json PATH writes the rows there.

    python tools/temporal_probe.py [--reps 5] [--no-quality] [--json PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CENTRE = (278.0, 278.0, 278.0)


def orbit(rt, w, h, spp, k):
    """The cornell_box view turned k degrees around the room's centre."""
    a = math.radians(k)
    eye = (CENTRE[0] + 1078.0 * math.sin(a), 278.0, CENTRE[2] - 1078.0 * math.cos(a))
    cam = rt.derive_camera(w, w / (h + 0.25), spp=spp, max_depth=10, vfov=40.0, lookfrom=eye, lookat=CENTRE)
    assert cam.image_height == h
    return cam


def quality(rt, r, w=200, frames=8, spp=16):
    import numpy as np

    rows = []
    t = r.temporal(w, w)
    for k in range(frames):
        cam = orbit(rt, w, w, spp, k)
        p = r.progressive(cam, seed=21 + k)
        linear, _, noise = p.step(spp)
        p.close()
        g = r.guides(cam, 4)
        out, out_se, _, n = t.accumulate(cam, linear, g, noise)
        truth, _, _ = r.render_host(orbit(rt, w, w, 1024, k), seed=1021)
        mse = lambda img: float(((img - truth) ** 2).sum(-1).mean())  # noqa: E731
        den_acc, den_one = r.denoise_guided(out, g, out_se)[0], r.denoise_guided(linear, g, noise)[0]
        rows.append({"what": "quality", "size": [w, w], "frame": k, "mean_history": round(float(n.mean()), 3), "share_with_history": round(float((n > 1).mean()), 4),
                     "mse_frame": mse(linear), "mse_accumulated": mse(out), "ratio": round(mse(out) / mse(linear), 4),
                     "mse_filtered_frame": mse(den_one), "mse_filtered_accumulated": mse(den_acc), "ratio_filtered": round(mse(den_acc) / mse(den_one), 4)})
    t.close()
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--json", default="", help="write the result rows to this file")
    args = ap.parse_args()

    import torch

    import raytracingoneweekendapplication_amd as rt

    lib = rt.hip_lib()
    r = rt.Renderer(0)
    rows = []
    tmp = tempfile.mkdtemp()
    earth = rt.write_synthetic_earth(os.path.join(tmp, "earth_synth.ppm"))
    scene = rt.Scene.build("cornell_box", rt.SCENE_SEED, earth)
    r.upload_fast(scene, scene.camera().center)

    def timed(fn):
        times = []
        for rep in range(args.reps + 1):                          # rep 0: warm-up
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn(rep)
            t1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(t0.elapsed_time(t1))
        return statistics.median(times), min(times), max(times)

    def check(rc):
        if rc != 0:
            raise rt.RtkError(rc, lib.rtk_last_error().decode())

    for W, H in ((1920, 1080), (800, 800)):
        for real_mode, dt, label in ((rt.RTK_REAL_F64, torch.float64, "f64"), (rt.RTK_REAL_F32, torch.float32, "f32")):
            cams = [orbit(rt, W, H, 16, k) for k in (0, 1)]
            opts = rt.RenderOpts(rt.RENDER_SEED, real_mode, 0, 1, 0, 0, None)
            guides = [torch.zeros((H, W, 16), dtype=torch.float32, device="cuda") for _ in cams]
            lin, noise = torch.zeros((H, W, 3), dtype=dt, device="cuda"), torch.zeros((H, W), dtype=torch.float32, device="cuda")
            for cam, g in zip(cams, guides):
                check(lib.rtk_render_guides(r._ctx, C.byref(cam), C.byref(opts), 4, None, g.data_ptr()))
            p = r.progressive(cams[0], real_mode=real_mode)
            p.step_device(16, lin.data_ptr(), 0, noise.data_ptr(), 0)
            torch.cuda.synchronize()
            p.close()
            out, o_se = torch.zeros_like(lin), torch.zeros_like(noise)
            u8, o_n = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda"), torch.zeros_like(noise)
            t = r.temporal(W, H, real_mode)
            t.accumulate_device(cams[0], lin.data_ptr(), guides[0].data_ptr(), noise.data_ptr())
            med, lo, hi = timed(lambda rep: t.accumulate_device(cams[(rep + 1) % 2], lin.data_ptr(), guides[(rep + 1) % 2].data_ptr(), noise.data_ptr(),
                                                                 out.data_ptr(), o_se.data_ptr(), u8.data_ptr(), o_n.data_ptr()))
            share = float((o_n > 1).float().mean())
            t.close()
            rows.append({"what": "temporal pass", "real": label, "size": [W, H], "median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                         "share_with_history": round(share, 4)})
            d = rt.DenoiseOpts(1, 0, 0, 0, 0, 0)
            med, lo, hi = timed(lambda rep: check(lib.rtk_denoise_guided(r._ctx, W, H, real_mode, lin.data_ptr(), guides[0].data_ptr(), noise.data_ptr(), C.byref(d), 0,
                                                                         out.data_ptr(), u8.data_ptr(), None)))
            rows.append({"what": "guided filter, 1 iteration", "real": label, "size": [W, H], "median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3)})
            med, lo, hi = timed(lambda rep: check(lib.rtk_render_guides(r._ctx, C.byref(cams[0]), C.byref(opts), 4, None, guides[0].data_ptr())))
            rows.append({"what": "guide pass, 4 spp", "real": label, "size": [W, H], "median_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3)})
            for row in rows[-3:]:
                print(f"{W}x{H} {label} {row['what']:>28}: median {row['median_ms']:8.3f} ms  (min {row['min_ms']:.3f}, max {row['max_ms']:.3f})"
                      + (f"  history on {row['share_with_history']:.3f} of the pixels" if "share_with_history" in row else ""), flush=True)
    if not args.no_quality:
        for row in quality(rt, r):
            rows.append(row)
            print("quality " + json.dumps(row), flush=True)
    r.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
