"""CPU test of csrc/rtk_grid_plan.h, the host arithmetic behind plan_launch (rtk_trace.hip): the grid of a persistent render
launch and the grid cap of variant bits 5..7.  tests/helpers/grid_plan_check.cpp -- a stand-alone program over the header alone,
built with the address and undefined-behaviour sanitizers and run directly -- computes the plan of every input of the grid

  CUs 1..304 x register-limited waves per CU 1..40 x kMaxWavesPerBlock 4, 8, 16 x workgroups per CU that LDS allows 1..8
  x n_items 1, 2, 63, 64, 65, 4095, 4096, 4097, 10^6 x cap 0..7            (21 012 480 plans)

and `ref_uncapped` / `ref_capped` below state the rule a second time, in numpy over the whole grid at once:

  uncapped  what plan_launch computed before the cap existed (its arithmetic restated line by line);
  always    threads a positive multiple of 64 and at most 64 x kMaxWavesPerBlock, blocks >= 1;
  cap k     blocks x threads / 64 <= 2^(k-1), == 2^(k-1) whenever the uncapped plan had at least that many waves, and never more
            waves than the uncapped plan.
"""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

PKG = os.path.join(ROOT, "raytracingoneweekendapplication_amd")
CUS = np.arange(1, 305)
WAVES = np.arange(1, 41)
MAX_WPB = np.array([4, 8, 16])
BY_LDS = np.arange(1, 9)
N_ITEMS = np.array([1, 2, 63, 64, 65, 4095, 4096, 4097, 10 ** 6])
CAPS = np.arange(0, 8)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("grid_plan") / "grid_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "helpers", "grid_plan_check.cpp"), "-I" + os.path.join(PKG, "csrc"), "-o", path])
    return path


def ask(exe, lines):
    p = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    out = [tuple(int(x) for x in line.split()) for line in p.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def ref_uncapped(cus, waves, max_wpb, by_lds, n_items):
    """plan_launch before the cap: -> (blocks, threads, waves per block); by_lds = 0: the kernel stages nothing."""
    waves_per_cu = np.clip(waves, 4, 32)
    blocks_per_cu = (waves_per_cu + max_wpb - 1) // max_wpb
    blocks_per_cu = np.where((by_lds > 0) & (blocks_per_cu > by_lds), by_lds, blocks_per_cu)
    wpb = np.maximum(np.minimum(waves_per_cu // blocks_per_cu, max_wpb), 1)
    needed = (n_items + wpb - 1) // wpb
    blocks = np.maximum(np.minimum(cus * blocks_per_cu, needed), 1)
    return blocks, wpb * 64, wpb


def ref_capped(blocks, threads, wpb, cap):
    """The cap on an uncapped plan: more than 2^(cap-1) waves become exactly that many, fewer are left alone."""
    limit = np.where(cap > 0, 1 << np.maximum(cap - 1, 0), 0)
    over = (cap > 0) & (blocks * wpb > limit)
    pow2 = 1 << np.floor(np.log2(wpb)).astype(np.int64)      # (wpb <= 16: exact)
    one_block = over & (limit < wpb)
    many = over & ~one_block
    out_blocks = np.where(one_block, 1, np.where(many, limit // pow2, blocks))
    out_threads = np.where(one_block, limit * 64, np.where(many, pow2 * 64, threads))
    return out_blocks, out_threads, limit


def test_every_plan_of_the_grid(exe):
    p = subprocess.run([exe, "sweep"], capture_output=True)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    shape = (len(CUS), len(WAVES), len(MAX_WPB), len(BY_LDS), len(N_ITEMS), len(CAPS))
    got = np.frombuffer(p.stdout, np.int32)
    assert got.size == 2 * int(np.prod(shape))
    got = got.reshape(shape + (2,)).astype(np.int64)
    waves, max_wpb, by_lds, n_items, cap = np.meshgrid(WAVES, MAX_WPB, BY_LDS, N_ITEMS, CAPS, indexing="ij")
    for k, cus in enumerate(CUS):       # one CU count at a time: 69 120 plans, a few MB of temporaries
        blocks, threads = got[k, ..., 0], got[k, ..., 1]
        u_blocks, u_threads, wpb = ref_uncapped(cus, waves, max_wpb, by_lds, n_items)
        # the uncapped output is the parent's
        assert np.array_equal(blocks[cap == 0], u_blocks[cap == 0]) and np.array_equal(threads[cap == 0], u_threads[cap == 0]), cus
        # the shape of any launch
        assert (threads > 0).all() and (threads % 64 == 0).all() and (threads <= 64 * max_wpb).all() and (blocks >= 1).all(), cus
        # the cap: the properties, then the second statement of the rule
        n_waves, u_waves = blocks * threads // 64, u_blocks * u_threads // 64
        r_blocks, r_threads, limit = ref_capped(u_blocks, u_threads, wpb, cap)
        capped = cap > 0
        assert (n_waves[capped] <= limit[capped]).all(), cus
        assert (n_waves[capped & (u_waves >= limit)] == limit[capped & (u_waves >= limit)]).all(), cus
        assert (n_waves <= u_waves).all(), cus
        assert np.array_equal(blocks, r_blocks) and np.array_equal(threads, r_threads), cus


def test_single_plans_and_the_cap_table(exe):
    assert ask(exe, [f"cap {k}" for k in range(8)]) == [(0,), (1,), (2,), (4,), (8,), (16,), (32,), (64,)]
    # a kernel that stages nothing (LDS limit 0 = none) on 256 CUs, 8 waves per CU in one workgroup: the 45 items of a 37 x 21
    # frame at 5 spp in chunks of 2 -- six workgroups of 8 waves uncapped, one workgroup of 1, 2, 4 waves at caps 1, 2, 3
    assert ask(exe, [f"plan 256 8 8 0 45 {k}" for k in range(4)]) == [(6, 512), (1, 64), (1, 128), (1, 256)]
    # ... and with sixteen waves per CU as two workgroups of 8: cap 5 (16 waves) is two workgroups, cap 7 (64) changes nothing
    assert ask(exe, ["plan 256 16 8 0 45 0", "plan 256 16 8 0 45 5", "plan 256 16 8 0 45 7"]) == [(6, 512), (2, 512), (6, 512)]
    # a workgroup of 5 waves (5 per CU, one workgroup): the capped grid is made of 4-wave workgroups so that it divides the cap
    assert ask(exe, ["plan 8 5 8 1 1000000 0", "plan 8 5 8 1 1000000 4", "plan 8 5 8 1 1000000 3"]) == [(8, 320), (2, 256), (1, 256)]


def test_frame_launches_and_names_do_not_read_the_cap(rt):
    """rtk_frame_launches answers from the camera and the options on the host: the same with every cap; a null context has no
    kernel name with or without one."""
    import ctypes as C

    lib = rt.hip_lib()
    cam = rt.derive_camera(1920, 16.0 / 9.0, spp=1000)
    for base, want in ((0, 3), (1 << 24, 1)):        # include/rtk.h: 1920 x 1080 at 1000 spp is three launches; bit 24: one
        for k in range(8):
            opts = rt.RenderOpts(1, rt.RTK_REAL_F64, 0, 1, 0, base | (k << 5), None)
            assert lib.rtk_frame_launches(C.byref(cam), C.byref(opts)) == want, (base, k)
    assert lib.rtk_kernel_name(None, rt.RTK_REAL_F64, 3 << 5) == b"" and lib.rtk_view_kernel_name(None, rt.RTK_REAL_F64, 3 << 5) == b""
