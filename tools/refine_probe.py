"""What refining an upsampled frame through a tile list costs (rtk_tiles_select, rtk_render_tiles).

At 1920x1080, f64, fast order, 16 spp, on cornell_box and book1_final, in one run: the full-resolution frame (rtk_render_device);
the support map of a half-resolution frame upsampled (rtk_upsample, factor 2); for refine_below 0.5 and 0.25 (dilate 1) the share
of tiles flagged and the times of the select, of rtk_render_tiles over those tiles, and of the three calls (upsample, select,
render_tiles) together -- beside the full frame's time x that share, what the tiles would cost if a tile list cost nothing.  Then
rtk_render_tiles over evenly spread tiles at fixed shares from 1 % (324 tiles: what a persistent-wave launch over a few hundred
tiles costs) to all of them, and the break-even share: the smallest share, interpolated between the measured ones, at which the
tile render takes as long as the full frame.  Device events around synchronised work, one warm-up, --reps timed runs, the median;
the variants alternate inside each repetition.  Prints one line per row; --json PATH writes the rows there.

    python tools/refine_probe.py [--reps 7] [--json PATH]
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

W, H, SPP, DEPTH = 1920, 1080, 16, 10
SHARES = (0.01, 0.02, 0.05, 0.1, 0.25, 0.5, 0.75, 1.0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default="", help="write the result rows to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import raytracingoneweekendapplication_amd as rt

    r = rt.Renderer(0)
    tmp = tempfile.mkdtemp()
    earth = rt.write_synthetic_earth(os.path.join(tmp, "earth_synth.ppm"))
    rows = []

    def timed(fns):
        """{name: (median, min, max) ms} of the callables, alternating inside each repetition (rep 0: warm-up)."""
        times = {k: [] for k in fns}
        for rep in range(args.reps + 1):
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                if rep:
                    times[k].append(t0.elapsed_time(t1))
        return {k: (round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)) for k, v in times.items()}

    n_tiles = rt.tiles_per_rank(W, H, 1)
    for name in ("cornell_box", "book1_final"):
        scene = rt.Scene.build(name, rt.SCENE_SEED, earth)
        full = scene.camera(W, H, SPP, DEPTH)
        r.upload_fast(scene, full.center)
        low = rt.upsample_camera(full, 2)
        LW, LH = low.image_width, low.image_height
        dev = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
        out, o_se, u8, o_sup = dev((H, W, 3), torch.float64), dev((H, W), torch.float32), dev((H, W, 3), torch.uint8), dev((H, W), torch.float32)
        g, low_g = dev((H, W, 16), torch.float32), dev((LH, LW, 16), torch.float32)
        low_lin, low_se = dev((LH, LW, 3), torch.float64), dev((LH, LW), torch.float32)
        flags, info = dev((n_tiles,), torch.int32), dev((2,), torch.int32)
        p = r.progressive(low)
        p.step_device(SPP, low_lin.data_ptr(), 0, low_se.data_ptr(), 0)
        torch.cuda.synchronize()
        p.close()
        r.guides_device(full, 4, g.data_ptr())
        r.guides_device(low, 4, low_g.data_ptr())
        torch.cuda.synchronize()

        def upsample():
            r.upsample_device(full, low_lin.data_ptr(), low_se.data_ptr(), low_g.data_ptr(), g.data_ptr(), out.data_ptr(), o_se.data_ptr(), u8.data_ptr(), o_sup.data_ptr())

        def render_tiles():
            r.render_tiles_device(full, flags.data_ptr(), out.data_ptr(), u8.data_ptr(), o_se.data_ptr(), o_sup.data_ptr(), info.data_ptr())

        upsample()
        torch.cuda.synchronize()
        support = o_sup.clone()
        base = {"scene": name, "size": [W, H], "real": "f64", "spp": SPP, "tiles": n_tiles}
        for below in (0.5, 0.25):
            def select():
                r.tiles_select_device(W, H, support.data_ptr(), 0, flags.data_ptr(), below=below, dilate=1)

            def three_calls():
                upsample()
                r.tiles_select_device(W, H, o_sup.data_ptr(), 0, flags.data_ptr(), below=below, dilate=1)
                render_tiles()

            select()
            torch.cuda.synchronize()
            flagged = int((flags != 0).sum())
            t = timed({"full": lambda: r.render_device(full, out.data_ptr()), "select": select, "render_tiles": render_tiles, "upsample": upsample,
                       "three_calls": three_calls})
            select()                                               # (three_calls selected on its own support map: the same flags)
            torch.cuda.synchronize()
            assert flagged == int((flags != 0).sum()) == int(info[1])
            share = flagged / n_tiles
            row = dict(base, what="refinement", refine_below=below, dilate=1, flagged=flagged, share=round(share, 4), full_ms=t["full"][0], select_ms=t["select"][0],
                       render_tiles_ms=t["render_tiles"][0], upsample_ms=t["upsample"][0], three_calls_ms=t["three_calls"][0], full_times_share_ms=round(t["full"][0] * share, 3),
                       spread={k: list(v) for k, v in t.items()})
            row["render_tiles_over_full_times_share"] = round(row["render_tiles_ms"] / max(row["full_times_share_ms"], 1e-9), 3)
            rows.append(row)
            print(f"{name} below {below}: {flagged} of {n_tiles} tiles ({share:.3f}); full {row['full_ms']:.3f} ms, x share {row['full_times_share_ms']:.3f}; select "
                  f"{row['select_ms']:.3f}, render_tiles {row['render_tiles_ms']:.3f}, upsample {row['upsample_ms']:.3f}, three calls {row['three_calls_ms']:.3f} ms", flush=True)
        # evenly spread tiles at fixed shares
        fns = {"full": lambda: r.render_device(full, out.data_ptr())}
        curve = []
        for share in SHARES:
            k = max(1, round(share * n_tiles))
            f = np.zeros(n_tiles, np.int32)
            f[np.unique(np.linspace(0, n_tiles - 1, k).round().astype(np.int64))] = 1
            flags.copy_(torch.from_numpy(f).to("cuda"))
            torch.cuda.synchronize()
            t = timed({"full": fns["full"], "render_tiles": render_tiles})
            curve.append({"share": round(int(f.sum()) / n_tiles, 4), "flagged": int(f.sum()), "render_tiles_ms": t["render_tiles"][0], "min_ms": t["render_tiles"][1],
                          "max_ms": t["render_tiles"][2], "full_ms": t["full"][0]})
            print(f"{name} spread {curve[-1]['flagged']} tiles ({curve[-1]['share']:.3f}): render_tiles {t['render_tiles'][0]:.3f} ms, full {t['full'][0]:.3f} ms", flush=True)
        full_ms = statistics.median(c["full_ms"] for c in curve)
        break_even = None
        for a, b in zip(curve, curve[1:]):
            if a["render_tiles_ms"] < full_ms <= b["render_tiles_ms"]:
                break_even = a["share"] + (b["share"] - a["share"]) * (full_ms - a["render_tiles_ms"]) / (b["render_tiles_ms"] - a["render_tiles_ms"])
        rows.append(dict(base, what="render_tiles over evenly spread tiles", full_ms=round(full_ms, 3), curve=curve,
                         break_even_share=None if break_even is None else round(break_even, 3),
                         note="break_even_share null: the tile render stayed below the full frame's time at every share" if break_even is None else ""))
        print(f"{name}: break-even share {break_even}", flush=True)
    r.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
