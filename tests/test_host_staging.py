"""The optional outputs of the *_host entry points.  A *_host call stages its buffers in one device allocation cut into pieces
(csrc/rtk_internal.h, HostStaging); an output the caller leaves null gets no piece, so which outputs are asked for moves every
piece behind it.  For each entry point with optional outputs, a call that asks for one output alone must return exactly the
bytes the all-outputs call returns for it, in both real modes.

The image is 13 x 9: 2 x 2 tiles, partial in both axes, and 13 * 9 * 3 * 4 bytes is no multiple of 16, so a piece laid out at
a wrong offset lands on a wrong address.  Upsampling uses factor 3 (a 5 x 3 low image).  Inputs are the analytic ones of
tests/rule_inputs.py through the neighbouring tests' generators.  Temporal and display objects are stateful: every call gets
a fresh object (temporal: brought to the same one-frame history first)."""
import ctypes as C

import numpy as np
import pytest

from tests.rule_inputs import rich_filter_case
from tests.test_display import _opts as display_opts
from tests.test_display import display_case
from tests.test_temporal import rich_frames
from tests.test_upsample import rich_case

W, H, FACTOR = 13, 9, 3
LINEAR, NOISE, RGB8 = ((H, W, 3), np.float64), ((H, W), np.float32), ((H, W, 3), np.uint8)


def _denoise(rt, renderer, real_mode, guided):
    lib = rt.hip_lib()
    linear, guides, se = rich_filter_case(H, W)
    linear, guides = np.ascontiguousarray(linear), np.ascontiguousarray(guides if guided else guides[..., :8])
    opts = rt.DenoiseOpts(2, 0, 0, 0, 0, 0)

    def call(outs):   # (the arrays live as long as this closure)
        head = (renderer._ctx, W, H, real_mode, linear.ctypes.data, guides.ctypes.data, se.ctypes.data, C.byref(opts))
        if guided:
            return lib.rtk_denoise_guided_host(*head, rt.DENOISE_DEMODULATE, *outs)
        return lib.rtk_denoise_host(*head, *outs)

    return call, {"linear": LINEAR, "rgb8": RGB8}


def _temporal(rt, renderer, real_mode):
    lib = rt.hip_lib()
    (cam0, colour0, g0, se0), (cam1, colour1, g1, se1) = rich_frames(rt, "orbit", W, H)[:2]
    opts = rt.TemporalOpts(0, 0, 0, 0, rt.TEMPORAL_CHECK_ALBEDO, 0)

    def call(outs):
        t = renderer.temporal(W, H, real_mode)
        try:
            t.accumulate(cam0, colour0, g0, se0)
            return lib.rtk_temporal_accumulate_host(t._h, C.byref(cam1), colour1.ctypes.data, g1.ctypes.data, se1.ctypes.data, C.byref(opts), *outs)
        finally:
            t.close()

    return call, {"linear": LINEAR, "noise": NOISE, "rgb8": RGB8, "history": NOISE}


def _upsample(rt, renderer, real_mode):
    lib = rt.hip_lib()
    full, colour, se, low_g, g = rich_case(rt, W, H, FACTOR)
    assert colour.shape == (3, 5, 3)
    opts = rt.UpsampleOpts(FACTOR, 0, 0, 0, rt.UPSAMPLE_DEMODULATE, 0)

    def call(outs):
        return lib.rtk_upsample_host(renderer._ctx, C.byref(full), real_mode, colour.ctypes.data, se.ctypes.data, low_g.ctypes.data, g.ctypes.data, C.byref(opts), *outs)

    return call, {"linear": LINEAR, "noise": NOISE, "rgb8": RGB8, "support": NOISE}


def _display(rt, renderer, real_mode):
    lib = rt.hip_lib()
    img = display_case(W, H)
    opts = display_opts(rt, curve=rt.DISPLAY_ACES, encode=rt.DISPLAY_SRGB, bloom=0.5, bloom_levels=2)

    def call(outs):
        d = renderer.display(W, H, real_mode)
        try:
            return lib.rtk_display_apply_host(d._h, img.ctypes.data, C.byref(opts), *outs)
        finally:
            d.close()

    return call, {"linear": LINEAR, "rgb8": RGB8}


ENTRY_POINTS = {"rtk_denoise_host": lambda *a: _denoise(*a, guided=False), "rtk_denoise_guided_host": lambda *a: _denoise(*a, guided=True),
                "rtk_temporal_accumulate_host": _temporal, "rtk_upsample_host": _upsample, "rtk_display_apply_host": _display}


@pytest.mark.gpu
@pytest.mark.parametrize("real_mode", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_one_output_alone_equals_its_bytes_among_all_outputs(rt, renderer, entry, real_mode):
    lib = rt.hip_lib()
    call, outputs = ENTRY_POINTS[entry](rt, renderer, real_mode)

    def run(wanted):
        bufs = {name: np.full(shape, 77, dtype) for name, (shape, dtype) in outputs.items() if name in wanted}
        assert call([bufs[name].ctypes.data if name in bufs else None for name in outputs]) == 0, lib.rtk_last_error()
        return bufs

    every = run(set(outputs))
    for name in outputs:
        assert (every[name] != 77).any(), name       # the call wrote it
        alone = run({name})[name]
        assert alone.tobytes() == every[name].tobytes(), (entry, name, int((alone != every[name]).sum()))
