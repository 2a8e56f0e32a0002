"""What the display transform costs, and how far noise moves its meter (rtk_display).

Times at 1920x1080, f64 and f32, on a rendered cornell_box frame (--spp, default 64: nearly every pixel is counted, most of them in
a few bins) -- device events around --inner frames enqueued back to back, one warm-up, --reps timed windows, the median, per frame:
  apply             a frame with a manual exposure and no bloom: the set-exposure launch and the apply kernel, with the cheapest
                    (CLAMP, GAMMA2) and the dearest (ACES, SRGB: three double pow per pixel) curve and encoding
  histogram+meter   a metered frame minus the one above: the histogram pass and the one-wave metering kernel
  meter (bound)     a whole metered frame of a 1x1 object (3 launches): an upper bound for the metering kernel, whose work does not
                    depend on the image
  bloom 4 / 6       a frame with bloom at 4 / 6 levels minus the same frame without
Each is also given as a fraction of its modelled bytes ("Display transform") over the machine's measured stream-copy
rate (rtk_microbench), with the launches per frame.  Then, on cornell_box and book2_final at 960x540 and 4, 16, 64 and 256 spp: the
metered exposure, and the share of pixels with a channel at 255 under the reference's conversion and under ACES with the metered
exposure.  Prints one line per row; --json PATH writes the rows there.

    python tools/display_probe.py [--reps 5] [--inner 20] [--json PATH] [--no-scenes]
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


def level_sizes(w: int, h: int, n: int):
    out = []
    for _ in range(n):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append(w * h)
    return out


def modelled_bytes(w: int, h: int, elem: int, levels: int = 0) -> dict:
    """Bytes each pass has to move for a w x h frame of `elem`-byte reals; the pyramid is 16-byte texels."""
    px = w * h
    m = {"histogram": 3 * elem * px, "apply": (6 * elem + 3) * px}
    if levels:
        t = level_sizes(w, h, levels)
        down = 3 * elem * px + 16 * t[0] + sum(16 * (t[k - 1] + t[k]) for k in range(1, levels))
        tents = sum(4 * 16 * n for n in t)
        up = sum(16 * (2 * t[k] + t[k + 1]) for k in range(levels - 1))
        m["bloom"] = down + tents + up + 16 * t[0]                # ... and the apply kernel's taps of level 1
    return m


def launches(levels: int, metered: bool = True) -> int:
    return (2 if metered else 1) + 1 + (3 * levels + levels - 1 if levels else 0)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=64, help="samples per pixel of the timed frame")
    ap.add_argument("--inner", type=int, default=20, help="frames enqueued back to back inside one timed window")
    ap.add_argument("--json", default="", help="write the result rows to this file")
    ap.add_argument("--no-scenes", action="store_true", help="skip the exposure-against-noise rows")
    args = ap.parse_args()

    import numpy as np
    import torch

    import raytracingoneweekendapplication_amd as rt

    copy_GBps = rt.microbench(0)["hbm_copy_GBps"]
    print(f"stream copy: {copy_GBps:.0f} GB/s   library: {rt.HIP_LIB_PATH}", flush=True)
    r = rt.Renderer(0)
    rows = [{"what": "stream copy", "GBps": round(copy_GBps, 1), "library": os.path.basename(rt.HIP_LIB_PATH)}]
    tmp = tempfile.mkdtemp()
    earth = rt.write_synthetic_earth(os.path.join(tmp, "earth_synth.ppm"))
    scenes = {name: rt.Scene.build(name, rt.SCENE_SEED, earth) for name in ("cornell_box", "book2_final")}

    def timed(fn):
        times = []
        for rep in range(args.reps + 1):                          # rep 0: warm-up
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.inner):
                fn()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(t0.elapsed_time(t1) / args.inner)
        return statistics.median(times)

    W, H = 1920, 1080
    scene = scenes["cornell_box"]
    r.upload_fast(scene, scene.camera().center)
    frame = r.render_host(scene.camera(W, H, args.spp, 10))[0]
    for real_mode, dt, label, elem in ((rt.RTK_REAL_F64, torch.float64, "f64", 8), (rt.RTK_REAL_F32, torch.float32, "f32", 4)):
        x = torch.from_numpy(frame).to("cuda", dtype=dt)
        out, u8 = torch.zeros((H, W, 3), dtype=dt, device="cuda"), torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        one_in, one_out = torch.ones((1, 1, 3), dtype=dt, device="cuda"), torch.zeros((1, 1, 3), dtype=dt, device="cuda")
        d, d1 = r.display(W, H, real_mode), r.display(1, 1, real_mode)
        run = lambda **o: timed(lambda: d.apply_device(x.data_ptr(), out.data_ptr(), u8.data_ptr(), curve=rt.DISPLAY_ACES, encode=rt.DISPLAY_SRGB, **o))  # noqa: E731
        t_manual = run(exposure=1.0)
        t_cheap = timed(lambda: d.apply_device(x.data_ptr(), out.data_ptr(), u8.data_ptr(), exposure=1.0))
        t_metered = run()
        t_one = timed(lambda: d1.apply_device(one_in.data_ptr(), one_out.data_ptr(), 0))
        t_bloom = {n: (run(bloom=0.5, bloom_levels=n), run(exposure=1.0, bloom=0.5, bloom_levels=n)) for n in (4, 6)}
        hist = d.histogram()
        base = {"real": label, "size": [W, H]}
        floor = lambda nbytes: nbytes / (copy_GBps * 1e9) * 1e3       # noqa: E731
        m = modelled_bytes(W, H, elem)
        passes = [("apply (CLAMP, GAMMA2)", t_cheap, m["apply"], launches(0, False)), ("apply (ACES, SRGB)", t_manual, m["apply"], launches(0, False)), ("histogram+meter", t_metered - t_manual, m["histogram"], 1),
                  ("meter (bound: a metered 1x1 frame)", t_one, 0, 3), ("metered frame, no bloom", t_metered, m["histogram"] + m["apply"], launches(0))]
        for n in (4, 6):
            mb = modelled_bytes(W, H, elem, n)
            passes.append(("bloom %d levels" % n, t_bloom[n][1] - t_manual, mb["bloom"], launches(n, False) - launches(0, False)))
            passes.append(("metered frame, bloom %d levels" % n, t_bloom[n][0], mb["histogram"] + mb["apply"] + mb["bloom"], launches(n)))
        for what, ms, nbytes, n_launch in passes:
            row = dict(base, what=what, median_ms=round(ms, 4), launches=n_launch)
            if nbytes:
                row.update(modelled_MB=round(nbytes / 1e6, 2), copy_floor_ms=round(floor(nbytes), 4), fraction_of_copy_rate=round(floor(nbytes) / ms, 3) if ms > 0 else None)
            rows.append(row)
            print(f"{W}x{H} {label} {what}: {ms:.4f} ms, {n_launch} launches" + (f", {row['fraction_of_copy_rate']} of the copy rate ({nbytes / 1e6:.1f} MB)" if nbytes else ""),
                  flush=True)
        top = np.sort(hist)[::-1]
        rows.append(dict(base, what="histogram of the timed frame", spp=args.spp, counted=int(hist.sum()), bins_used=int((hist > 0).sum()),
                         share_in_top_bin=round(float(top[0]) / max(1, int(hist.sum())), 4), share_in_top_4_bins=round(float(top[:4].sum()) / max(1, int(hist.sum())), 4)))
        print(rows[-1], flush=True)
        d.close()
        d1.close()

    if not args.no_scenes:
        w, h = 960, 540
        for name, scene in scenes.items():
            r.upload_fast(scene, scene.camera().center)
            d = r.display(w, h)
            for spp in (4, 16, 64, 256):
                linear, rgb8, _ = r.render_host(scene.camera(w, h, spp, 10))
                d.reset()
                _, aces8, e = d.apply(linear, curve=rt.DISPLAY_ACES)
                row = {"what": "metered exposure against noise", "scene": name, "size": [w, h], "spp": spp, "exposure": round(e, 6),
                       "clipped_reference": round(float((rgb8 == 255).any(-1).mean()), 5), "clipped_aces_metered": round(float((aces8 == 255).any(-1).mean()), 5)}
                rows.append(row)
                print(row, flush=True)
            d.close()
    r.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
