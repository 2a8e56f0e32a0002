"""CPU test of the LDS image of the MIXED program (rtk_device_layout.h MixedImg) on the library's sphere-only
scenes, through the host-only entry rtk_debug_mixed_program: the image must hold the records in memory value for value and
link for link -- the kernel that stages it and the one that reads memory then test the same boxes and spheres -- with every
head unit's kind in the low nibble of word 3 as kind ^ 1 and every box's link usable as read."""
import ctypes as C

import numpy as np
import pytest

from tests.scene_cases import SCENE_SEED
from tests.test_gpu_parity import _spheres_of

OP_END, OP_BOX, OP_SPHERE, OP_SPHERE_MOVING = 0, 1, 2, 9
UNITS = {OP_END: 1, OP_BOX: 1, OP_SPHERE: 2, OP_SPHERE_MOVING: 3}


def mixed_program(rt, scene, eye):
    fn = rt.hip_lib().rtk_debug_mixed_program
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    fast = scene.fast_order(eye)
    eye_extent = max(abs(eye.x), abs(eye.y), abs(eye.z))
    n, extent = C.c_int32(0), C.c_float(0)
    assert fn(fast.desc_ptr, eye_extent, 0, C.byref(n), C.byref(extent), None, None) == 0, rt.hip_lib().rtk_last_error()
    units, image = np.zeros((n.value, 8), np.uint32), np.zeros((n.value, 8), np.uint32)
    small = np.zeros((1, 8), np.uint32)
    assert fn(fast.desc_ptr, eye_extent, 1, C.byref(n), C.byref(extent), small.ctypes.data, None) != 0 and not small.any()  # too small: refused, untouched
    assert fn(fast.desc_ptr, eye_extent, n.value, C.byref(n), C.byref(extent), units.ctypes.data, image.ctypes.data) == 0
    return units, image, float(extent.value)


def heads(units):
    pc = 0
    while pc < len(units):
        kind = int(units[pc, 6]) & 15
        yield pc, kind
        pc += UNITS[kind]
    assert pc == len(units)


def check_image(units, image):
    kinds = {}
    for pc, kind in heads(units):
        u, m = units[pc], image[pc]
        kinds[kind] = kinds.get(kind, 0) + 1
        assert (int(m[3]) & 15) ^ 1 == kind, (pc, kind)   # every head tells its kind at word 3
        if kind == OP_BOX:
            link = int(u[7])
            assert link % 32 == 0 and 0 < link <= 32 * (len(units) - 1)
            assert np.array_equal(m[0:3], u[0:3]) and int(m[3]) == link and np.array_equal(m[4:7], u[3:6]) and m[7] == u[6], pc
        else:
            assert np.array_equal(m[0:2], u[0:2]) and m[2] == u[7] and int(m[3]) == int(u[6]) ^ 1 and np.array_equal(m[4:8], u[2:6]), pc
            for k in range(1, UNITS[kind]):
                assert np.array_equal(image[pc + k], units[pc + k])   # continuation units as they are
    return kinds


@pytest.mark.parametrize("name", ["book1_final", "three_spheres"])
def test_library_scene_image_equals_the_records_in_memory(rt, name):
    scene = rt.Scene.build(name, SCENE_SEED)
    cam = scene.camera(64, 36, 1, 4)
    units, image, extent = mixed_program(rt, scene, cam.center)
    kinds = check_image(units, image)
    assert kinds[OP_END] == 1 and kinds[OP_BOX] > 0 and kinds[OP_SPHERE] == len(_spheres_of(scene)) and extent > 0


def test_moving_spheres_keep_their_three_units(rt):
    scene = rt.Scene.build("three_spheres", SCENE_SEED)
    spheres = _spheres_of(scene)
    spheres[1].center_dir[0], spheres[3].center_dir[2] = 0.3, -0.25
    units, image, _ = mixed_program(rt, scene, scene.camera(64, 36, 1, 4).center)
    kinds = check_image(units, image)
    assert kinds[OP_SPHERE_MOVING] == 2 and kinds[OP_SPHERE] == len(spheres) - 2
