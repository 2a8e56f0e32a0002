"""What rendering a frame in progressive steps costs against the one-shot frame (rtk_progressive_* vs rtk_render_device).

Every step is its own render launch (LDS staging of the program per workgroup, the drain of its last long paths) plus one pass of
rtk_accumulate_kernel over the session's planes.  This probe times, on the frames bench.py times (fast order, full size):
  C2 (book1_final 1920x1080x100): one-shot vs steps of 8, 32 and 100 samples;
  C5 (book2_final 1920x1080x1000): one-shot vs steps of 64 samples.
Device events around the whole frame (session creation -- allocation and zeroing -- is outside), one warm-up frame per
variant, --reps timed frames; prints one line per variant and, with --json PATH, writes the rows there.  Every frame's image
is checked against the one-shot image (sha256 of the f64 linear buffer).

    python tools/progressive_probe.py [--reps 5] [--configs c2,c5] [--json PATH]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANS = {"c2": ("book1_final", [8, 32, 100]), "c5": ("book2_final", [64])}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--json", default="", help="write the result rows to this file")
    args = ap.parse_args()

    import torch

    import raytracingoneweekendapplication_amd as rt

    r = rt.Renderer(0)
    results = []
    tmp = tempfile.mkdtemp()
    for cfg in args.configs.split(","):
        name, step_sizes = PLANS[cfg]
        scene = rt.Scene.build(name, rt.SCENE_SEED, rt.write_synthetic_earth(os.path.join(tmp, "earth_synth.ppm")))
        cam = scene.camera()
        r.upload_fast(scene, cam.center)
        W, H, spp = cam.image_width, cam.image_height, cam.samples_per_pixel
        lin = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        noise = torch.zeros((H, W), dtype=torch.float32, device="cuda")

        def one_shot():
            r.render_device(cam, lin.data_ptr(), u8.data_ptr())

        def stepped(n):
            def run(p):
                while p.samples_done < spp:
                    p.step_device(min(n, spp - p.samples_done), lin.data_ptr(), u8.data_ptr(), noise.data_ptr())
            return run

        variants = [("one-shot", None, one_shot)] + [(f"steps of {n}", n, stepped(n)) for n in step_sizes]
        base_ms = None
        ref_sha = None
        for label, n, fn in variants:
            times = []
            for rep in range(args.reps + 1):                      # rep 0: warm-up
                p = r.progressive(cam) if n else None
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn(p) if n else fn()
                t1.record()
                torch.cuda.synchronize()
                if p:
                    p.close()
                if rep:
                    times.append(t0.elapsed_time(t1))
            sha = hashlib.sha256(lin.cpu().numpy().tobytes()).hexdigest()[:16]
            ref_sha = ref_sha or sha
            med = statistics.median(times)
            base_ms = base_ms or med
            row = {"config": cfg, "scene": name, "size": [W, H, spp], "variant": label, "steps": -(-spp // n) if n else 1,
                   "median_ms": round(med, 2), "min_ms": round(min(times), 2), "max_ms": round(max(times), 2),
                   "vs_one_shot": round(med / base_ms, 3), "framebuffer_sha256": sha, "identical": sha == ref_sha}
            results.append(row)
            print(f"{cfg} {label:>12}: {row['steps']:3d} step(s)  median {med:8.2f} ms  (min {min(times):.2f}, max {max(times):.2f}, "
                  f"n={len(times)})  x{row['vs_one_shot']:.3f}  sha {sha} {'ok' if row['identical'] else 'DIFFERENT'}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    if not all(row["identical"] for row in results):
        raise SystemExit("a stepped frame differs from the one-shot frame")


if __name__ == "__main__":
    main()
