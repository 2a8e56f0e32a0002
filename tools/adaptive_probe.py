"""What tile-adaptive sampling saves against uniform progressive steps (rtk_progressive_set_adaptive vs plain steps).

On the frames bench.py times at their stated sizes (fast order): C3 (cornell_box 800x800x1000) and C5 (book2_final
1920x1080x1000), for every --rel-targets value, two runs with the same step size and min_samples:
  (a) uniform: plain steps until every tile has met the retire rule once (the largest se / max(m, 1e-3) of its in-image pixels
      <= rel_target at a step end with min_samples <= samples_done < target; computed from each step's noise map and preview)
      or the target is reached;
  (b) adaptive: the same rel_target, step size and min_samples, until the target or until no tile is active.
A warm-up frame of each run fixes its number of steps (and, for (b), the active tiles after each step); --reps timed frames
replay them with device events around every step (session creation is outside).  Reported per run: pixel-samples rendered,
device ms of the frame, and per step the active tiles before it and its median ms.  Every retired tile of (b) is checked
against (a)'s preview at the tile's count wherever (a) passed through that count (bit for bit).

    python tools/adaptive_probe.py [--reps 5] [--configs c3,c5] [--rel-targets 0.1,0.05] [--step 64] [--min-samples 64] [--json PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"c3": "cornell_box", "c5": "book2_final"}


def tile_metric(torch, lin, noise, W, H):
    """[ty, tx] float64: the retire metric of every tile from a preview and its se map."""
    m = lin.mean(dim=2)  # = S1 / K: the mean of the chunk means (r + g + b) / 3
    rel = noise.double() / torch.clamp(m, min=1e-3)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    pad = torch.zeros((ty * 8, tx * 8), dtype=torch.float64, device=rel.device)
    pad[:H, :W] = rel
    return pad.reshape(ty, 8, tx, 8).amax(dim=(1, 3))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--rel-targets", default="0.1,0.05")
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--min-samples", type=int, default=64)
    ap.add_argument("--json", default="", help="write the result rows to this file")
    args = ap.parse_args()

    import torch

    import raytracingoneweekendapplication_amd as rt

    r = rt.Renderer(0)
    results = []
    tmp = tempfile.mkdtemp()
    ok = True
    for cfg in args.configs.split(","):
        name = SCENES[cfg]
        scene = rt.Scene.build(name, rt.SCENE_SEED, rt.write_synthetic_earth(os.path.join(tmp, "earth_synth.ppm")))
        cam = scene.camera()
        r.upload_fast(scene, cam.center)
        W, H, spp = cam.image_width, cam.image_height, cam.samples_per_pixel
        tx, ty = (W + 7) // 8, (H + 7) // 8
        lin = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        noise = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        px = torch.zeros((ty * 8, tx * 8), dtype=torch.int64)
        px[:H, :W] = 1
        tile_px = px.reshape(ty, 8, tx, 8).sum(dim=(1, 3)).reshape(-1)
        for rel_target in (float(x) for x in args.rel_targets.split(",")):
            step, min_samples = args.step, args.min_samples

            def timed(make, n_steps):
                """--reps frames of n_steps steps after creation: (frame ms medians, per-step ms medians)."""
                frames, per_step = [], [[] for _ in range(n_steps)]
                for _ in range(args.reps):
                    p = make()
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_steps + 1)]
                    torch.cuda.synchronize()
                    ev[0].record()
                    for k in range(n_steps):
                        p.step_device(min(step, spp - p.samples_done), lin.data_ptr(), 0, noise.data_ptr())
                        ev[k + 1].record()
                    torch.cuda.synchronize()
                    p.close()
                    frames.append(ev[0].elapsed_time(ev[-1]))
                    for k in range(n_steps):
                        per_step[k].append(ev[k].elapsed_time(ev[k + 1]))
                return frames, [statistics.median(t) for t in per_step]

            # (a) warm-up / analysis: uniform steps until every tile has met the rule once
            p = r.progressive(cam)
            met = torch.zeros((ty, tx), dtype=torch.bool, device="cuda")
            previews = {}
            while p.samples_done < spp:
                p.step_device(min(step, spp - p.samples_done), lin.data_ptr(), 0, noise.data_ptr())
                s = p.samples_done
                previews[s] = lin.clone()
                if min_samples <= s < spp:
                    met |= tile_metric(torch, lin, noise, W, H) <= rel_target
                    if bool(met.all()):
                        break
            n_a, done_a = len(previews), p.samples_done
            p.close()
            # (b) warm-up: the adaptive run, its active tiles per step and its tile map
            p = r.progressive(cam, rel_target=rel_target, min_samples=min_samples)
            active = [p.adaptive_status()["active_tiles"]]
            while p.samples_done < spp and active[-1] > 0:
                p.step_device(min(step, spp - p.samples_done), lin.data_ptr(), 0, noise.data_ptr())
                active.append(p.adaptive_status()["active_tiles"])
            n_b = len(active) - 1
            tile_spp = torch.from_numpy(p.tile_samples())
            st = p.adaptive_status()
            p.close()
            smap = tile_spp.reshape(ty, tx).repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W].cuda()
            checked = mismatched = 0
            for s in torch.unique(tile_spp[tile_spp < done_a]).tolist():
                if s in previews:
                    sel = smap == s
                    checked += int((tile_spp == s).sum())
                    mismatched += int((lin[sel] != previews[s][sel]).any(dim=-1).sum())
            previews.clear()
            ok = ok and mismatched == 0
            fa, sa = timed(lambda: r.progressive(cam), n_a)
            fb, sb = timed(lambda: r.progressive(cam, rel_target=rel_target, min_samples=min_samples), n_b)
            row = {"config": cfg, "scene": name, "size": [W, H, spp], "rel_target": rel_target, "step": step, "min_samples": min_samples,
                   "tiles": tx * ty,
                   "uniform": {"steps": n_a, "samples_done": done_a, "all_tiles_met": done_a < spp or bool(met.all()),
                               "pixel_samples": W * H * done_a, "median_ms": round(statistics.median(fa), 2), "min_ms": round(min(fa), 2),
                               "max_ms": round(max(fa), 2), "step_ms": [round(t, 2) for t in sa]},
                   "adaptive": {"steps": n_b, "pixel_samples": int(st["pixel_samples"]), "mean_spp": round(st["mean_spp"], 2),
                                "retired_tiles": st["retired_tiles"], "median_ms": round(statistics.median(fb), 2), "min_ms": round(min(fb), 2),
                                "max_ms": round(max(fb), 2), "active_before_step": active[:-1], "step_ms": [round(t, 2) for t in sb]},
                   "retired_tiles_checked": checked, "retired_tiles_differing": mismatched}
            row["pixel_samples_ratio"] = round(row["adaptive"]["pixel_samples"] / row["uniform"]["pixel_samples"], 3)
            row["ms_ratio"] = round(row["adaptive"]["median_ms"] / row["uniform"]["median_ms"], 3)
            results.append(row)
            print(f"{cfg} rel_target {rel_target}: uniform {n_a} steps to {done_a} spp, {row['uniform']['pixel_samples'] / 1e6:.1f} M px-samples, "
                  f"{row['uniform']['median_ms']:.1f} ms | adaptive {n_b} steps, mean {st['mean_spp']:.1f} spp, "
                  f"{row['adaptive']['pixel_samples'] / 1e6:.1f} M px-samples, {row['adaptive']['median_ms']:.1f} ms  "
                  f"(x{row['pixel_samples_ratio']} samples, x{row['ms_ratio']} time) | retired tiles checked {checked}, differing {mismatched}",
                  flush=True)
            print(f"    adaptive active tiles before each step {active[:-1]}", flush=True)
            print(f"    adaptive ms per step {[round(t, 1) for t in sb]}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    if not ok:
        raise SystemExit("a retired tile differs from the uniform run's preview at its count")


if __name__ == "__main__":
    main()
