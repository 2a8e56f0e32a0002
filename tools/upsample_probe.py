"""What guided upsampling costs and what it saves (rtk_upsample).

Times, on C3 (cornell_box) in the fast order, f64 and f32, at 1920x1080 and 800x800, factors 2 and 4, in one run: the upsample
pass (all four outputs; plain and demodulated), the 16-spp render and the 4-sample guide pass of the low camera, and beside them
the 16-spp render and the guide pass at full resolution -- device events around synchronised work, one warm-up, --reps timed
runs, the median.  The statement under test: low render + low guides + full guides + upsample < full render + full guides, at
equal samples per pixel.  The pass is also given as a fraction of its modelled bytes ("Guided upsampling") over the
machine's measured stream-copy rate (rtk_microbench).  Prints one line per row; --json PATH writes the rows there.

    python tools/upsample_probe.py [--reps 5] [--json PATH]
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


def modelled_bytes_per_pixel(f: int, elem: int) -> float:
    """Bytes per FULL pixel the pass has to move: its guides in, the low-resolution pixel (colour, se, guides) once per f^2 full
    pixels in, the four outputs out.  The depth-gradient neighbours are other lanes' guide lines."""
    return 64.0 + (3 * elem + 4 + 64) / (f * f) + (3 * elem + 4 + 3 + 4)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default="", help="write the result rows to this file")
    args = ap.parse_args()

    import torch

    import raytracingoneweekendapplication_amd as rt

    lib = rt.hip_lib()
    copy_GBps = rt.microbench(0)["hbm_copy_GBps"]
    print(f"stream copy: {copy_GBps:.0f} GB/s", flush=True)
    r = rt.Renderer(0)
    rows = [{"what": "stream copy", "GBps": round(copy_GBps, 1)}]
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
            fn()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                times.append(t0.elapsed_time(t1))
        return round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)

    def check(rc):
        if rc != 0:
            raise rt.RtkError(rc, lib.rtk_last_error().decode())

    for W, H in ((1920, 1080), (800, 800)):
        for real_mode, dt, label in ((rt.RTK_REAL_F64, torch.float64, "f64"), (rt.RTK_REAL_F32, torch.float32, "f32")):
            full = scene.camera(W, H, 16, 10)
            opts = rt.RenderOpts(rt.RENDER_SEED, real_mode, 0, 1, 0, 0, None)
            g = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda")
            out, o_se = torch.zeros((H, W, 3), dtype=dt, device="cuda"), torch.zeros((H, W), dtype=torch.float32, device="cuda")
            u8, o_sup = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda"), torch.zeros((H, W), dtype=torch.float32, device="cuda")
            base = {"real": label, "size": [W, H]}
            t_render = timed(lambda: r.render_device(full, out.data_ptr(), real_mode=real_mode))
            t_guides = timed(lambda: check(lib.rtk_render_guides(r._ctx, C.byref(full), C.byref(opts), 4, None, g.data_ptr())))
            rows.append(dict(base, what="full render, 16 spp", median_ms=t_render[0], min_ms=t_render[1], max_ms=t_render[2]))
            rows.append(dict(base, what="full guide pass, 4 spp", median_ms=t_guides[0], min_ms=t_guides[1], max_ms=t_guides[2]))
            print(f"{W}x{H} {label}: full render {t_render[0]:.3f} ms, full guides {t_guides[0]:.3f} ms", flush=True)
            for f in (2, 4):
                low = rt.upsample_camera(full, f)
                LW, LH = low.image_width, low.image_height
                low_lin, low_se = torch.zeros((LH, LW, 3), dtype=dt, device="cuda"), torch.zeros((LH, LW), dtype=torch.float32, device="cuda")
                low_g = torch.zeros((LH, LW, 16), dtype=torch.float32, device="cuda")
                p = r.progressive(low, real_mode=real_mode)       # the low frame with its se, as a caller makes it
                p.step_device(16, low_lin.data_ptr(), 0, low_se.data_ptr(), 0)
                torch.cuda.synchronize()
                p.close()
                t_low = timed(lambda: r.render_device(low, low_lin.data_ptr(), real_mode=real_mode))
                t_low_g = timed(lambda: check(lib.rtk_render_guides(r._ctx, C.byref(low), C.byref(opts), 4, None, low_g.data_ptr())))
                row = dict(base, factor=f, low_size=[LW, LH], low_render_ms=t_low[0], low_guides_ms=t_low_g[0], full_render_ms=t_render[0], full_guides_ms=t_guides[0])
                for demodulate in (False, True):
                    t_up = timed(lambda: r.upsample_device(full, low_lin.data_ptr(), low_se.data_ptr(), low_g.data_ptr(), g.data_ptr(), out.data_ptr(), o_se.data_ptr(),
                                                           u8.data_ptr(), o_sup.data_ptr(), real_mode=real_mode, factor=f, demodulate=demodulate))
                    key = "upsample_demodulated" if demodulate else "upsample"
                    row.update({key + "_ms": t_up[0], key + "_min_ms": t_up[1], key + "_max_ms": t_up[2]})
                bpp = modelled_bytes_per_pixel(f, 8 if real_mode == rt.RTK_REAL_F64 else 4)
                floor_ms = bpp * W * H / (copy_GBps * 1e9) * 1e3
                row.update(what="upsampled frame", modelled_bytes_per_pixel=round(bpp, 2), copy_floor_ms=round(floor_ms, 4),
                           fraction_of_copy_rate=round(floor_ms / row["upsample_ms"], 3), mean_support=round(float(o_sup.mean()), 4),
                           upsampled_total_ms=round(t_low[0] + t_low_g[0] + t_guides[0] + row["upsample_ms"], 3), full_total_ms=round(t_render[0] + t_guides[0], 3))
                row["upsampled_over_full"] = round(row["upsampled_total_ms"] / row["full_total_ms"], 4)
                rows.append(row)
                print(f"{W}x{H} {label} f={f}: low render {t_low[0]:.3f} + low guides {t_low_g[0]:.3f} + full guides {t_guides[0]:.3f} + upsample "
                      f"{row['upsample_ms']:.3f} (demodulated {row['upsample_demodulated_ms']:.3f}) = {row['upsampled_total_ms']:.3f} ms against "
                      f"{row['full_total_ms']:.3f} ms; the pass at {row['fraction_of_copy_rate']:.2f} of the copy rate ({bpp:.1f} B/px)", flush=True)
    r.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
