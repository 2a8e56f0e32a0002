"""What the denoiser costs and what it buys, at 1920x1080 (rtk_render_aovs, rtk_denoise, rtk_progressive_denoise and their
guided forms rtk_render_guides, rtk_denoise_guided, rtk_progressive_denoise_guided).

Times, on C2 (book1_final) and C3 (cornell_box) at their bench size in the fast order, f64:
  the AOV pass at 1, 4 and 16 samples per pixel, and the filter at its defaults (5 iterations) and at 1 and 8 iterations,
the guide pass (4 samples; following mirrors, and mirrors and glass) and the guided filter (plain and demodulating) beside them,
with device events around synchronised work (one warm-up, --reps timed runs, the median).  Then the quality numbers of
tests/test_denoise.py at full size: a 32-spp progressive preview, denoised with 4-sample AOVs, against a 1024-spp frame of
another seed -- the mean squared error of the noisy and the denoised image over all pixels and over "edge" pixels (3x3 depth
range > 5 % of the depth, or a normal cosine < 0.9), and the same ratio for the guided and the demodulating filter, over all
pixels and over the pixels where a guide sample followed a mirror.  Prints one line per row; --json PATH writes the rows there.

    python tools/denoise_probe.py [--reps 5] [--configs c2,c3] [--no-quality] [--json PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"c2": "book1_final", "c3": "cornell_box"}


def _clamped(x, oy, ox):
    import numpy as np

    h, w = x.shape[:2]
    return x[np.clip(np.arange(h) + oy, 0, h - 1)][:, np.clip(np.arange(w) + ox, 0, w - 1)]


def quality(rt, r, scene, w, h):
    import numpy as np

    cam = scene.camera(w, h, 32, 10)
    p = r.progressive(cam)
    noisy, _, _ = p.step(32)
    den, _ = p.denoised(4)
    guided = {"guided": p.denoised_guided(4)[0], "demodulated": p.denoised_guided(4, demodulate=True)[0],
              "guided_glass": p.denoised_guided(4, follow=3)[0], "demodulated_glass": p.denoised_guided(4, follow=3, demodulate=True)[0]}
    p.close()
    truth, _, _ = r.render_host(scene.camera(w, h, 1024, 10), seed=rt.RENDER_SEED + 1000)
    aov = r.aovs(cam, 4)
    z, n = aov[..., 7].astype(np.float64), aov[..., 4:7].astype(np.float64)
    around = [(b, a) for b in (-1, 0, 1) for a in (-1, 0, 1)]
    zr = np.max([_clamped(z, b, a) for b, a in around], 0) - np.min([_clamped(z, b, a) for b, a in around], 0)
    nn = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-12)
    cmin = np.min([(nn * _clamped(nn, b, a)).sum(-1) for b, a in around], 0)
    edge = (zr > 0.05 * z) | (cmin < 0.9)
    e0, e1 = ((noisy - truth) ** 2).sum(-1), ((den - truth) ** 2).sum(-1)
    q = {"mse_noisy": float(e0.mean()), "mse_denoised": float(e1.mean()), "ratio": round(float(e1.mean() / e0.mean()), 4),
         "edge_fraction": round(float(edge.mean()), 4), "edge_ratio": round(float(e1[edge].mean() / e0[edge].mean()), 4)}
    # pixels where a guide sample followed a mirror: the path goes on behind the first hit
    g = r.guides(cam, 4)
    mirror = (g[..., 3] == 1) & (g[..., 15] > g[..., 7])
    q["mirror_fraction"] = round(float(mirror.mean()), 4)
    if mirror.any():
        q["mirror_ratio"] = round(float(e1[mirror].mean() / e0[mirror].mean()), 4)
    for key, img in guided.items():
        e = ((img - truth) ** 2).sum(-1)
        q[key + "_ratio"] = round(float(e.mean() / e0.mean()), 4)
        if mirror.any():
            q[key + "_mirror_ratio"] = round(float(e[mirror].mean() / e0[mirror].mean()), 4)
    return q


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="c2,c3")
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
        return statistics.median(times), min(times), max(times)

    def check(rc):
        if rc != 0:
            raise rt.RtkError(rc, lib.rtk_last_error().decode())

    for cfg in args.configs.split(","):
        name = SCENES[cfg]
        scene = rt.Scene.build(name, rt.SCENE_SEED, earth)
        cam = scene.camera()
        r.upload_fast(scene, cam.center)
        W, H = cam.image_width, cam.image_height
        aov = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        lin = torch.rand((H, W, 3), dtype=torch.float64, device="cuda")
        noise = torch.rand((H, W), dtype=torch.float32, device="cuda") * 0.1
        out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        opts = rt.RenderOpts(rt.RENDER_SEED, rt.RTK_REAL_F64, 0, 1, 0, 0, None)
        for n in (1, 4, 16):
            med, lo, hi = timed(lambda: check(lib.rtk_render_aovs(r._ctx, C.byref(cam), C.byref(opts), n, aov.data_ptr())))
            rows.append({"config": cfg, "scene": name, "size": [W, H], "what": f"aov pass, {n} spp", "median_ms": round(med, 3),
                         "min_ms": round(lo, 3), "max_ms": round(hi, 3)})
        for it in (1, 5, 8):
            d = rt.DenoiseOpts(it, 0, 0, 0, 0, 0)
            med, lo, hi = timed(lambda: check(lib.rtk_denoise(r._ctx, W, H, rt.RTK_REAL_F64, lin.data_ptr(), aov.data_ptr(), noise.data_ptr(), C.byref(d),
                                                              out.data_ptr(), u8.data_ptr(), None)))
            rows.append({"config": cfg, "scene": name, "size": [W, H], "what": f"denoise, {it} iterations", "median_ms": round(med, 3),
                         "min_ms": round(lo, 3), "max_ms": round(hi, 3)})
        guides = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda")
        for follow, label in ((1, "mirrors"), (3, "mirrors + glass")):
            go = rt.GuideOpts(follow, 0)
            med, lo, hi = timed(lambda: check(lib.rtk_render_guides(r._ctx, C.byref(cam), C.byref(opts), 4, C.byref(go), guides.data_ptr())))
            rows.append({"config": cfg, "scene": name, "size": [W, H], "what": f"guide pass, 4 spp, {label}", "median_ms": round(med, 3),
                         "min_ms": round(lo, 3), "max_ms": round(hi, 3)})
        check(lib.rtk_render_guides(r._ctx, C.byref(cam), C.byref(opts), 4, None, guides.data_ptr()))
        d = rt.DenoiseOpts(5, 0, 0, 0, 0, 0)
        for flags, label in ((0, "guided denoise, 5 iterations"), (1, "guided + demodulate, 5 it.")):
            med, lo, hi = timed(lambda: check(lib.rtk_denoise_guided(r._ctx, W, H, rt.RTK_REAL_F64, lin.data_ptr(), guides.data_ptr(), noise.data_ptr(),
                                                                     C.byref(d), flags, out.data_ptr(), u8.data_ptr(), None)))
            rows.append({"config": cfg, "scene": name, "size": [W, H], "what": label, "median_ms": round(med, 3), "min_ms": round(lo, 3),
                         "max_ms": round(hi, 3)})
        for row in rows[-10:]:
            print(f"{cfg} {row['what']:>30}: median {row['median_ms']:8.3f} ms  (min {row['min_ms']:.3f}, max {row['max_ms']:.3f})", flush=True)
        if not args.no_quality:
            q = quality(rt, r, scene, W, H)
            rows.append(dict({"config": cfg, "scene": name, "size": [W, H], "what": "quality, 32 spp vs 1024 spp"}, **q))
            print(f"{cfg} quality: {json.dumps(q)}", flush=True)
    r.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
