"""The table of rtk_render_kernel<real, FEAT, COUNT, IN_LDS> instantiations (csrc/rtk_trace.hip): one row per instantiation
that kernel_choice::choose (csrc/rtk_kernel_choice.h) can select, with a scene, an upload order, a real mode, a variant word and count_work that select it.
Data and scene builders only -- the tests are in test_abi_and_host.py (the compiled set == the table, CPU) and
test_kernel_matrix.py (every row rendered on the device, and the dispatched names read back from a kernel trace).

FEAT is the sum of rtk_device_layout.h's feature bits: F_QUAD 1, F_TRI 2, F_XFORM 4, F_MEDIA 8, F_TEXTURE 16, F_LIGHTS 32,
F_EXOTIC_MAT 64, F_FMA_BOX 128, F_F32_BOX 256, F_MATTE 512, F_LDS_BOXES 1024, F_SPHERE_MEDIA_ONLY 2048; the families are
lean 0, mesh 66, quad/box 69, full 127.
"""
import collections
import csv
import glob
import os
import random
import re
import subprocess

from tests.desc_builder import DescBuilder
from tests.scene_cases import IMAGE_CASES, SCENE_SEED, scene_file

F64, F32 = "f64", "f32"
REFERENCE, FAST = "reference", "fast"          # rtk_scene_upload / rtk_scene_upload_fast (F_FMA_BOX, MIXED / COMPACT programs)
# variant bits that kernel_choice::choose reads
V_GLOBAL = 1                # bit 0: the program stays in global memory (allow_lds = false)
V_SLOT = 1 << 20            # the slot program although the upload built a MIXED / COMPACT one
V_NO_LDS_BOXES = 1 << 21    # no F_LDS_BOXES
V_COLD = 1 << 23            # the hot/cold form of the COMPACT program although the whole would fit

WIDTH, HEIGHT, SPP = 37, 21, 3   # ragged tiles (5 x 3 tiles of 8 x 8) and one partial sample chunk
MAX_DEPTH = 10

Row = collections.namedtuple("Row", "scene order real variant count expect note")


def _row(scene, order, real, variant, count, feat, in_lds, note=""):
    return Row(scene, order, real, variant, count, (real, feat, count, in_lds), note)


def row_id(row):
    return f"{row.scene}-{row.order}-{row.real}-v{row.variant:#x}" + ("-count" if row.count else "")


def kernel_name(expect):
    """What rtk_kernel_name prints (kernel_choice::format_name, rtk_kernel_choice.h) and a kernel trace shows behind `rtk::`."""
    real, feat, count, in_lds = expect
    return f"rtk_render_kernel<{'double' if real == F64 else 'float'}, {feat}u, {'true' if count else 'false'}, {'true' if in_lds else 'false'}>"


# ------------------------------------------------------------------------------------------------ scenes
# The nine IMAGE_CASES scenes wherever one selects the family; built here only what none of them does:
#   quadbox_metal     quads, a box() instance, spheres, one metal: the quad/box family WITHOUT F_MATTE (cornell_box is matte)
#   mesh_metal_small  triangles + spheres with a metal: the mesh family without F_MATTE (mesh and obj_mesh are both matte)
#   mesh_metal_large  the same with 1 700 triangles: slot programs larger than one CU's 163 840 B of LDS in BOTH real types
#                     (6 140 slots: 392 960 B in f64, 196 480 B in f32; fast order 5 925 slots: 379 200 / 189 600 B -- `mesh`,
#                     4 618 slots, is 295 552 B in f64 but 147 776 B in f32 and fits) whose box tables still fit (119 240 /
#                     70 112 B; fast order 145 632 / 85 128 B): F_LDS_BOXES on the mesh family, f32 included
#   sphere_fog        a fog ball inside one STATIONARY sphere among other spheres: F_SPHERE_MEDIA_ONLY with a COMPACT program that
#                     fits LDS (single_fog's boundary moves, cornell_smoke's are boxes: both keep the generic medium bracket;
#                     book2_final has the flag but its COMPACT program does not fit)
N_LARGE_TRIANGLES = 1700
CUSTOM_DEPTH = 8


def _quadbox_metal():
    b = DescBuilder()
    white, red, green = b.lambertian((0.73, 0.73, 0.73)), b.lambertian((0.65, 0.05, 0.05)), b.lambertian((0.12, 0.45, 0.15))
    steel, lamp = b.metal((0.8, 0.8, 0.9), 0.05), b.light((7.0, 7.0, 6.0))
    top = [b.quad((-3, -1, -8), (6, 0, 0), (0, 0, 6), white),       # floor
           b.quad((-3, -1, -8), (6, 0, 0), (0, 4, 0), steel),        # a mirror for a back wall
           b.quad((-3, -1, -8), (0, 0, 6), (0, 4, 0), red),
           b.quad((3, -1, -8), (0, 0, 6), (0, 4, 0), green),
           b.quad((-1, 2.9, -6), (2, 0, 0), (0, 0, 2), lamp),
           b.sphere((1.3, -0.4, -4.0), 0.6, steel),
           b.sphere((-1.6, -0.6, -3.5), 0.4, white)]
    x0, y0, z0, x1, y1, z1 = -0.6, -1.0, -0.6, 0.6, 0.7, 0.6        # box(a, b): six quads (quad.h:71-90), here around the origin
    dx, dy, dz = (x1 - x0, 0, 0), (0, y1 - y0, 0), (0, 0, z1 - z0)
    sides = [b.quad((x0, y0, z1), dx, dy, white), b.quad((x1, y0, z1), (0, 0, -dz[2]), dy, white), b.quad((x1, y0, z0), (-dx[0], 0, 0), dy, white),
             b.quad((x0, y0, z0), dz, dy, white), b.quad((x0, y1, z1), dx, (0, 0, -dz[2]), white), b.quad((x0, y0, z0), dx, dz, white)]
    top.append(b.translate(b.rotate_y(b.list(sides), 25.0), (-0.4, 0.0, -5.5)))
    return b.finish(b.list(top))


def _mesh_metal(n_triangles):
    rnd = random.Random(20251017 + n_triangles)
    b = DescBuilder()
    mats = [b.lambertian((0.7, 0.35, 0.2)), b.lambertian((0.3, 0.5, 0.7)), b.metal((0.8, 0.7, 0.6), 0.1)]
    members = [b.sphere((0, -101, -5), 100.0, b.lambertian((0.5, 0.5, 0.5))), b.sphere((2.5, 4.0, -3.0), 1.5, b.light((10.0, 10.0, 9.0))),
               b.sphere((0.0, 0.0, -4.0), 0.7, mats[2])]
    size = 0.9 if n_triangles < 100 else 0.3
    for i in range(n_triangles):
        c = (rnd.uniform(-3.5, 3.5), rnd.uniform(-0.9, 2.5), rnd.uniform(-8.0, -3.0))
        u = (rnd.uniform(0.4, 1.0) * size, rnd.uniform(-0.3, 0.3) * size, rnd.uniform(-0.4, 0.4) * size)
        v = (rnd.uniform(-0.3, 0.3) * size, rnd.uniform(0.4, 1.0) * size, rnd.uniform(-0.4, 0.4) * size)
        members.append(b.triangle(c, tuple(c[k] + u[k] for k in range(3)), tuple(c[k] + v[k] for k in range(3)), mats[i % 3]))
    return b.finish(b.list([b.bvh(members, rnd)]))


def _sphere_fog():
    b = DescBuilder()
    glass = b.dielectric(1.5)
    shell = b.sphere((-0.4, 0.1, -4.0), 1.0, glass)
    top = [b.sphere((0, -101, -5), 100.0, b.lambertian((0.5, 0.6, 0.4))), shell, b.medium(shell, 0.9, (0.2, 0.4, 0.9)),
           b.sphere((1.6, -0.3, -3.4), 0.6, b.metal((0.8, 0.7, 0.6), 0.0)), b.sphere((-2.2, -0.5, -3.0), 0.5, b.lambertian((0.7, 0.3, 0.2))),
           b.sphere((3.0, 4.0, -2.0), 1.2, b.light((8.0, 8.0, 7.0))), b.medium(b.sphere((1.0, 0.9, -5.5), 0.8, glass), 2.5, (0.9, 0.9, 0.9))]
    return b.finish(b.list(top))


CUSTOM_SCENES = {"quadbox_metal": _quadbox_metal, "sphere_fog": _sphere_fog, "mesh_metal_small": lambda: _mesh_metal(24),
                 "mesh_metal_large": lambda: _mesh_metal(N_LARGE_TRIANGLES)}
SCENE_DEPTH = {c[0]: min(c[4], MAX_DEPTH) for c in IMAGE_CASES}
SCENE_DEPTH.update({name: CUSTOM_DEPTH for name in CUSTOM_SCENES})


class MatrixScene:
    """A named scene of scene_library.h or one built here, behind the few members the tests use of rt.Scene."""

    def __init__(self, rt, name):
        from tests.conftest import GOLDEN

        self.name = name
        self.custom = name in CUSTOM_SCENES
        if self.custom:
            self._scene = CUSTOM_SCENES[name]()
            self._view = rt.Scene.build("three_spheres")   # its camera: at the origin, looking down -z, where these scenes lie
        else:
            self._scene = self._view = rt.Scene.build(name, SCENE_SEED, scene_file(name, GOLDEN))
        self._rt = rt

    @property
    def desc_ptr(self):
        return self._scene.desc_ptr

    def camera(self, width=WIDTH, height=HEIGHT, spp=SPP, depth=0):
        return self._view.camera(width, height, spp, depth or SCENE_DEPTH[self.name])

    def fast_order(self, eye):
        """The hierarchy rtk_scene_upload_fast renders, as a description the oracle can execute."""
        return self._rt.FastOrderScene(self._scene, eye)


def upload(renderer, scene, cam, order):
    """-> rtk_optimize_info of the fast order, None for the reference order."""
    if order == FAST:
        return renderer.upload_fast(scene, cam.center)
    renderer.upload(scene)
    return None


# ------------------------------------------------------------------------------------------------ rows
# COUNT = true rows: rtk_kernel_name always asks with count = false, so their tuples follow kernel_choice::kernel_features_base's counting rule
# (MIXED program on a lean scene: its own instantiation, staged like the timed one; COMPACT: full-feature | F_F32_BOX, in memory;
# slot program: full-feature | the order's F_FMA_BOX, in memory) and only the trace test confirms them.
_DUP_REF = "the all-in-memory twin of this scene's F_LDS_BOXES row: the f32 bit-identity of that row is this comparison"
ROWS = [
    # lean family (three_spheres: 1.6 KB of program)
    _row("three_spheres", REFERENCE, F64, 0, False, 0, True),
    _row("three_spheres", REFERENCE, F64, V_GLOBAL, False, 0, False),
    _row("three_spheres", REFERENCE, F32, 0, False, 0, True),
    _row("three_spheres", REFERENCE, F32, V_GLOBAL, False, 0, False),
    _row("three_spheres", FAST, F64, 0, False, 256, True),                      # MIXED
    _row("three_spheres", FAST, F64, V_GLOBAL, False, 256, False),
    _row("three_spheres", FAST, F64, 0, True, 256, True),
    _row("three_spheres", FAST, F64, V_GLOBAL, True, 256, False),
    _row("three_spheres", FAST, F64, V_SLOT, False, 128, True),
    _row("three_spheres", FAST, F64, V_SLOT | V_GLOBAL, False, 128, False),
    _row("three_spheres", FAST, F32, 0, False, 128, True),
    _row("three_spheres", FAST, F32, V_GLOBAL, False, 128, False),
    # quad/box family without F_MATTE (f64: kernel_choice::choose strips F_MATTE from f32, whose quad/box rows cornell_box serves)
    _row("quadbox_metal", REFERENCE, F64, 0, False, 69, True),
    _row("quadbox_metal", REFERENCE, F64, V_GLOBAL, False, 69, False),
    _row("quadbox_metal", FAST, F64, 0, False, 325, True),                      # COMPACT
    # quad/box family, matte
    _row("cornell_box", REFERENCE, F64, 0, False, 581, True),
    _row("cornell_box", REFERENCE, F64, V_GLOBAL, False, 581, False),
    _row("cornell_box", REFERENCE, F32, 0, False, 69, True),
    _row("cornell_box", REFERENCE, F32, V_GLOBAL, False, 69, False),
    _row("cornell_box", FAST, F64, 0, False, 837, True),
    # mesh family without F_MATTE, program in LDS or forced out of it (no box table: the program is small)
    _row("mesh_metal_small", REFERENCE, F64, 0, False, 66, True),
    _row("mesh_metal_small", REFERENCE, F64, V_GLOBAL, False, 66, False),
    _row("mesh_metal_small", FAST, F64, 0, False, 322, True),
    _row("mesh_metal_small", FAST, F64, V_SLOT, False, 194, True),
    _row("mesh_metal_small", FAST, F64, V_SLOT | V_GLOBAL, False, 194, False),
    # mesh family, matte (obj_mesh: two triangles)
    _row("obj_mesh", REFERENCE, F64, 0, False, 578, True),
    _row("obj_mesh", REFERENCE, F64, V_GLOBAL, False, 578, False),
    _row("obj_mesh", REFERENCE, F32, 0, False, 66, True),
    _row("obj_mesh", REFERENCE, F32, V_GLOBAL, False, 66, False),
    _row("obj_mesh", FAST, F64, 0, False, 834, True),
    _row("obj_mesh", FAST, F64, V_SLOT, False, 706, True),
    _row("obj_mesh", FAST, F64, V_SLOT | V_GLOBAL, False, 706, False),
    _row("obj_mesh", FAST, F32, 0, False, 194, True),
    _row("obj_mesh", FAST, F32, V_GLOBAL, False, 194, False),
    # mesh family, F_LDS_BOXES (slot program bytes: see mesh_metal_large above)
    _row("mesh_metal_large", REFERENCE, F64, 0, False, 66 | 1024, False),
    _row("mesh_metal_large", REFERENCE, F32, 0, False, 66 | 1024, False),
    _row("mesh_metal_large", REFERENCE, F32, V_NO_LDS_BOXES, False, 66, False, _DUP_REF),
    _row("mesh_metal_large", FAST, F64, V_SLOT, False, 194 | 1024, False),
    _row("mesh_metal_large", FAST, F32, 0, False, 194 | 1024, False),
    _row("mesh_metal_large", FAST, F32, V_NO_LDS_BOXES, False, 194, False, _DUP_REF),
    _row("mesh", REFERENCE, F64, 0, False, 578 | 1024, False),                  # 295 552 B of slot program (fast order: 256 192 B)
    _row("mesh", FAST, F64, V_SLOT, False, 706 | 1024, False),
    # full-feature family (material_zoo: no medium; sphere_fog: F_SPHERE_MEDIA_ONLY)
    _row("material_zoo", REFERENCE, F64, 0, False, 127, True),
    _row("material_zoo", REFERENCE, F64, V_GLOBAL, False, 127, False),
    _row("material_zoo", REFERENCE, F64, 0, True, 127, False),
    _row("material_zoo", REFERENCE, F32, 0, False, 127, True),
    _row("material_zoo", REFERENCE, F32, V_GLOBAL, False, 127, False),
    _row("material_zoo", REFERENCE, F32, 0, True, 127, False),
    _row("material_zoo", FAST, F64, 0, False, 383, True),
    _row("material_zoo", FAST, F64, 0, True, 383, False),
    _row("material_zoo", FAST, F64, V_SLOT, False, 255, True),
    _row("material_zoo", FAST, F64, V_SLOT | V_GLOBAL, False, 255, False),
    _row("material_zoo", FAST, F64, V_SLOT, True, 255, False),
    _row("material_zoo", FAST, F64, V_COLD, False, 383 | 1024, False),
    _row("material_zoo", FAST, F32, 0, False, 255, True),
    _row("material_zoo", FAST, F32, V_GLOBAL, False, 255, False),
    _row("material_zoo", FAST, F32, 0, True, 255, False),
    _row("sphere_fog", FAST, F64, 0, False, 383 | 2048, True),
    _row("sphere_fog", FAST, F64, V_COLD, False, 383 | 1024 | 2048, False),
    # full-feature family, F_LDS_BOXES (book2_final: 13 852 slots, 886 528 B in f64 and 443 264 B in f32; fast order 10 219 slots)
    _row("book2_final", REFERENCE, F64, 0, False, 127 | 1024, False),
    _row("book2_final", REFERENCE, F32, 0, False, 127 | 1024, False),
    _row("book2_final", REFERENCE, F32, V_NO_LDS_BOXES, False, 127, False, _DUP_REF),
    _row("book2_final", FAST, F64, V_SLOT, False, 255 | 1024, False),
    _row("book2_final", FAST, F32, 0, False, 255 | 1024, False),
    _row("book2_final", FAST, F32, V_NO_LDS_BOXES, False, 255, False, _DUP_REF),
]

# Work-counter slack of a COUNT row on a MIXED / COMPACT program (test_gpu_parity._assert_culling_counters, the values
# test_fast_order_on_the_device uses for the scene's class); rows on the slot program must equal the oracle's counters.
CULLING_SLACK = {"three_spheres": 0.03, "material_zoo": 0.25}

# Compiled instantiations that kernel_choice::choose cannot select: tuple -> the condition that excludes it.
UNREACHABLE = {}

# f32 sample coherence with the f64 kernel at spp = 1 (tests/test_f32_parity.py: TAU, COHERENT_P99 and the rule for the bound)
# of the (scene, order) pairs with f32 rows that test_f32_sample_coherence_with_f64 does not run:
# scene -> (observed reference order, observed fast order, bound = the larger observation x 2 + 0.5 %), on the MI355X at 37 x 21.
MATRIX_INCOHERENT = {
    "mesh_metal_large": (0.0, 0.0, 0.005),     # coherent_p99 3.97e-8 in both orders
}


# ------------------------------------------------------------------------------------------------ what was compiled, what ran
_LLVM = "/opt/rocm/lib/llvm/bin"
_MANGLED = re.compile(r"_ZN3rtk17rtk_render_kernelI([df])Lj(\d+)ELb([01])ELb([01])E")


def kernel_static_lds(hip_lib_path, tmp_dir):
    """{kernel symbol: .group_segment_fixed_size} of the gfx950 code object inside librtk_hip.so, from its metadata notes;
    None where ROCm's LLVM binary tools are missing."""
    tools = [os.path.join(_LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not all(os.path.exists(t) for t in tools):
        return None
    fat, dev = os.path.join(str(tmp_dir), "fat.bin"), os.path.join(str(tmp_dir), "dev.co")
    subprocess.check_call([tools[0], f"--dump-section=.hip_fatbin={fat}", hip_lib_path, os.path.join(str(tmp_dir), "copy.so")])
    subprocess.check_call([tools[1], "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={dev}", "--unbundle"])
    notes = subprocess.check_output([tools[2], "--notes", dev], text=True)
    sizes = {}
    fixed = None
    for line in notes.splitlines():
        m = re.search(r"\.group_segment_fixed_size:\s*(\d+)", line)
        if m:
            fixed = int(m.group(1))
        m = re.search(r"\.name:\s*(\S+)", line)
        if m and fixed is not None:
            sizes[m.group(1)] = fixed
            fixed = None
    return sizes


def compiled_instantiations(symbols):
    """The (real, FEAT, COUNT, IN_LDS) tuples among kernel symbols (as a list: a symbol is unique, so are these)."""
    out = []
    for s in symbols:
        m = _MANGLED.match(s)
        if m:
            out.append((F64 if m.group(1) == "d" else F32, int(m.group(2)), m.group(3) == "1", m.group(4) == "1"))
    return out


def dispatched_instantiations(trace_dir):
    """The tuples of the rtk::rtk_render_kernel<...> names in every kernel-trace CSV below `trace_dir`."""
    out = set()
    files = glob.glob(os.path.join(str(trace_dir), "**", "*kernel_trace.csv"), recursive=True)
    for path in files:
        with open(path, newline="") as f:
            for rec in csv.DictReader(f):
                m = re.search(r"rtk::rtk_render_kernel<(double|float), (\d+)u, (true|false), (true|false)>", rec["Kernel_Name"])
                if m:
                    out.add((F64 if m.group(1) == "double" else F32, int(m.group(2)), m.group(3) == "true", m.group(4) == "true"))
    return out, len(files)
