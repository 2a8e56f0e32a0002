"""The frame entry points (include/rtk.h: rtk_render_device / _host, view batches, tile lists, rtk_tiles_unpermute,
rtk_frame_launches, rtk_progressive_create, rtk_render_multi_enqueue) as a table in the style of tests/entry_faults.py, whose
Fault, Entry, fault and call it uses: for each of the 12 a good call of an 8x8 frame with 1 sample per pixel and the named faults
it can be given -- against three contexts: none ("null"), one without a scene ("empty") and one with three_spheres ("scene").

What differs from the lane-per-ray table, and how it is fitted to tests/golden/make_entry_refusals.py's transcript():
  * with a context the good call is accepted.  The library is seen through Answers, which gives an accepted call the return
    code ACCEPTED (1) and the text "<entry>: accepted" -- the terminal of the peel chains of the "scene" context -- and puts
    "<entry>: from " in front of a text that does not begin with the entry point's name (a host form's device form refused);
  * a fault the entry point does not refuse (a width of 65537 where no check bounds it) is `solo`: recorded alone, as accepted,
    and never part of a chain, so that no chain ends in a frame of two such faults;
  * an accepted call writes its outputs: the buffers are restored afterwards (Buffers.restore), so that untouched() at the end
    says that no REFUSED call wrote anything.

tests/golden/make_frame_refusals.py records what a library answers, tests/test_frame_refusals.py replays the record.
"""
import ctypes as C

import numpy as np

from tests.entry_faults import Entry, call, fault  # noqa: F401  (call: for the users of this table)

ACCEPTED = 1
RTK_ERR_HIP = -3
KINDS = ("null", "empty", "scene")
W = H = 8
BIG = 65537                                       # one past the largest image side of the image passes
FILL = 0x5A
# Byte offsets of the regions of a buffer block (64-byte multiples); the largest accepted frame is two views of 65537 x 8.
REGIONS = {"linear": 26 << 20, "rgb8": 4 << 20, "gathered": 13 << 20, "noise": 3 << 20, "support": 3 << 20, "flags": 64 << 10, "maps": 4 << 10, "info": 64,
           "counters": 256}


class Block:
    """REGIONS in one allocation, every byte FILL but the zeroed tile flags: numpy memory, or a torch tensor on the device."""

    def __init__(self, device):
        self.offset, at = {}, 0
        for name, size in REGIONS.items():
            self.offset[name] = at
            at += size
        self.size = at
        if device:
            import torch

            self.mem = torch.empty(at + 64, dtype=torch.uint8, device="cuda")
            address = self.mem.data_ptr()
        else:
            self.mem = np.empty(at + 64, np.uint8)
            address = self.mem.ctypes.data
        self.lo = (-address) % 64
        self.base = address + self.lo
        self.restore()

    def _region(self, name):
        return self.mem[self.lo + self.offset[name]:self.lo + self.offset[name] + REGIONS[name]]

    def restore(self):
        self.mem[:] = FILL
        self._region("flags")[:] = 0

    def untouched(self):                            # (compared eight bytes at a time: regions are 64-byte multiples on a 64-byte boundary)
        if isinstance(self.mem, np.ndarray):
            words = lambda r: r.view(np.uint64)  # noqa: E731
        else:
            import torch

            words = lambda r: r.view(torch.int64)  # noqa: E731
        return all(bool((words(self._region(n)) == (0 if n == "flags" else FILL * 0x0101010101010101)).all()) for n in REGIONS)

    def at(self, name, plus=0):
        return self.base + self.offset[name] + plus


class Buffers:
    """What every call points at: a block of host memory and a block of device memory (host memory where there is no device: a
    call with a null context touches neither)."""

    def __init__(self, device):
        self.device = device
        self.h, self.d = Block(False), Block(device)

    def restore(self):
        if self.device:
            import torch

            torch.cuda.synchronize()
        self.h.restore()
        self.d.restore()

    def untouched(self):
        return self.h.untouched() and self.d.untouched()


class Context:
    """One of KINDS: the rtk_ctx and the one-device rtk_multi the calls are given (None for "null")."""

    def __init__(self, rt, kind):
        self.kind, self.ctx, self.multi = kind, None, None
        if kind == "null":
            return
        self._renderer, self._multi = rt.Renderer(0), rt.MultiRenderer([0])
        if kind == "scene":
            scene = rt.Scene.build("three_spheres")
            self._renderer.upload(scene)
            self._multi.upload(scene)
        self.ctx, self.multi = self._renderer._ctx, self._multi._m


class Answers:
    """The library as entry_faults.call and transcript() see it (see the module's text)."""

    def __init__(self, lib):
        self.lib, self.entry, self.accepted = lib, "", False

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def rtk_last_error(self):
        text = self.lib.rtk_last_error().decode()
        if self.accepted:
            text = "accepted"
        elif text.startswith(self.entry + ": "):
            text = text[len(self.entry) + 2:]
        else:
            text = "from " + text
        return (self.entry + ": " + text).encode()


def _camera(rt, s, **changes):
    cam = rt.derive_camera(W, 1.0, spp=1, max_depth=5)
    assert (cam.image_width, cam.image_height) == (W, H)
    for field, key in (("image_width", "width"), ("image_height", "height"), ("samples_per_pixel", "spp"), ("max_depth", "max_depth")):
        setattr(cam, field, s[key])
    for field, v in changes.items():
        setattr(cam, field, v)
    return cam


def _opts(rt, s):
    return rt.RenderOpts(7, s["real_mode"], s["rank"][0], s["rank"][1], s["count_work"], s["variant"], None)


GOOD = {"b": lambda b: b, "cam": True, "opts": True, "width": W, "height": H, "spp": 1, "max_depth": 5, "rank": (0, 1), "real_mode": 0, "count_work": 0, "variant": 0}


def _entry(name, context, good, body, faults, terminal, after=None, writes=True):
    """`body(lib, rt, s)` makes the call; `after(lib, rt, s)` undoes what an accepted one leaves behind; writes: it is given buffers."""

    def invoke(lib, rt, s):
        lib.entry, lib.accepted = name, False
        rc = body(lib, rt, s)
        if rc >= 0:                                 # (rtk_frame_launches answers with a count)
            lib.accepted = True
            if after:
                after(lib, rt, s)
            if writes:
                s["b"].restore()
            return ACCEPTED
        if rc == RTK_ERR_HIP:                       # the runtime keeps its last error, and the next launch would report it as its own
            lib.hipGetLastError()
        return rc

    # (`context` itself is kept with the state: its handles live as long as the entry that passes them)
    return Entry(name, dict(GOOD, ctx=context.multi if "multi" in name else context.ctx, context=context, writes=writes, **good), invoke, faults,
                 {"null": terminal, "empty": "no scene uploaded", "scene": "accepted"}[context.kind] if isinstance(terminal, str) else terminal[context.kind])


def _camera_faults(names, bounded=False, depth_names=None, depth_solo=False):
    """Width and height of 0, negative and 65537, spp of 0 and 32768, max_depth of -1.  bounded: the entry point refuses 65537."""
    out = []
    for key in ("width", "height"):
        out += [fault(key + "_zero", key, {key: 0}, names), fault(key + "_negative", key, {key: -3}, names),
                fault(key + "_65537", key, {key: BIG}, names if bounded else "", solo=not bounded)]
    out += [fault("spp_zero", "spp", {"spp": 0}, names), fault("spp_32768", "spp", {"spp": 32768}, names),
            fault("max_depth_negative", "max_depth", {"max_depth": -1}, depth_names or names, solo=depth_solo)]
    return out


def _rank_faults(names, whole=None):
    """Rank pairs -1 of 1, 1 of 1 and 0 of 0.  whole: what an entry point that takes whole images says of 0 of 0."""
    return [fault("rank_negative", "rank", {"rank": (-1, 1)}, names), fault("rank_1_of_1", "rank", {"rank": (1, 1)}, names),
            fault("rank_0_of_0", "rank", {"rank": (0, 0)}, whole or names)]


REAL_MODE = [fault("real_mode_2", "real_mode", {"real_mode": 2}, "unknown real_mode"), fault("real_mode_negative", "real_mode", {"real_mode": -1}, "unknown real_mode")]
NULLS = [fault("null_cam", "cam", {"cam": False}, "null argument"), fault("null_opts", "opts", {"opts": False}, "null argument")]
BIT22 = 1 << 22


def _ref(on, obj):
    return C.byref(obj) if on else None


# ------------------------------------------------------------------------------------------- rtk_render_device / _host --
def _render(name, context):
    host = name.endswith("_host")
    good = {"linear": lambda b: (b.h if host else b.d).at("linear"), "rgb8": lambda b: (b.h if host else b.d).at("rgb8"), "counters": None}

    def body(lib, rt, s):
        return getattr(lib, name)(s["ctx"], _ref(s["cam"], _camera(rt, s)), _ref(s["opts"], _opts(rt, s)), s["linear"], s["rgb8"], s["counters"])

    faults = NULLS + _camera_faults("bad camera dimensions") + REAL_MODE + [fault("variant_bit_22", "variant", {"variant": BIT22}, "d_rgb8 must be null")]
    if host:                                        # the image is allocated before the device form sees the camera: a HIP failure, recorded alone
        faults = [f._replace(solo=True, names="") if f.name in ("width_negative", "height_negative") else f for f in faults]
        faults += _rank_faults("bad rank", "renders whole images") + [fault("n_ranks_2", "rank", {"rank": (0, 2)}, "renders whole images")]
    else:
        faults += _rank_faults("bad rank") + [fault("rgb8_with_n_ranks_2", "rank", {"rank": (0, 2)}, "d_rgb8 must be null"),
                                              fault("count_work_without_counters", "count_work", {"count_work": 1}, "count_work needs d_counters")]
    return _entry(name, context, good, body, faults, "null argument")


# ---------------------------------------------------------------------------------------------------------- view batches --
def _views(name, context):
    host = name.endswith("_host")
    good = {"n_views": 2, "view1": {}, "linear": lambda b: (b.h if host else b.d).at("linear"), "rgb8": lambda b: (b.h if host else b.d).at("rgb8"), "counters": None}

    def body(lib, rt, s):
        n = max(2, min(s["n_views"], 65536))
        cams = (rt.Camera * n)(*([_camera(rt, s)] * n))
        cams[1] = _camera(rt, s, **s["view1"])
        return getattr(lib, name)(s["ctx"], s["n_views"], cams if s["cam"] else None, None, _ref(s["opts"], _opts(rt, s)), s["linear"], s["rgb8"], s["counters"])

    differs = {"image_width": 16, "image_height": 16, "samples_per_pixel": 2, "pixel_samples_scale": 0.5}
    faults = NULLS + _camera_faults("bad camera dimensions", depth_names="negative max_depth") + REAL_MODE + _rank_faults("renders whole views") + [
        fault("n_ranks_2", "rank", {"rank": (0, 2)}, "renders whole views"), fault("variant_bit_22", "variant", {"variant": BIT22}, "variant bit 22"),
        fault("n_views_zero", "n_views", {"n_views": 0}, "n_views"), fault("n_views_65537", "n_views", {"n_views": 65537}, "n_views"),
        fault("view_1_max_depth_negative", "max_depth", {"view1": {"max_depth": -1}}, "view 1 has a negative max_depth")]
    faults += [fault("view_1_differs_in_" + k, "view1", {"view1": {k: v}}, "view 1 differs") for k, v in differs.items()]
    if not host:
        faults += [fault("count_work_without_counters", "count_work", {"count_work": 1}, "count_work needs d_counters"),
                   # 65536 views x 32768 tiles x 1 chunk = 2^31 work items: refused on host arithmetic, before anything is allocated
                   fault("work_items_2p31", "n_views", {"n_views": 65536, "width": 2048, "height": 1024}, solo=True)]
    return _entry(name, context, good, body, faults, "null argument")


# ------------------------------------------------------------------------------------------------------------ tile lists --
def _render_tiles(name, context):
    host = name.endswith("_host")
    side = (lambda b: b.h) if host else (lambda b: b.d)
    outs = ("linear", "rgb8", "noise", "support", "info")
    good = {"flags": lambda b: side(b).at("flags"), "max_tiles": 0}
    good.update({k: (lambda b, k=k: side(b).at(k)) for k in outs})

    def body(lib, rt, s):
        return getattr(lib, name)(s["ctx"], _ref(s["cam"], _camera(rt, s)), _ref(s["opts"], _opts(rt, s)), s["flags"], s["max_tiles"], *(s[k] for k in outs))

    p = "h_" if host else "d_"
    faults = [fault("null_cam", "cam", {"cam": False}, "null camera or options"), fault("null_opts", "opts", {"opts": False}, "null camera or options"),
              fault("null_flags", "flags", {"flags": None}, p + "tile_flags is null"), fault("max_tiles_negative", "max_tiles", {"max_tiles": -1}, "max_tiles -1 is negative"),
              fault("no_output", "out", {k: None for k in outs[:4]}, "no output", solo=True),
              fault("n_ranks_2", "rank", {"rank": (0, 2)}, "tile lists are one rank's"), fault("variant_bit_22", "variant", {"variant": BIT22}, "variant bit 22")]
    faults += _camera_faults("bad camera dimensions", bounded=host) + REAL_MODE + _rank_faults("tile lists are one rank's")
    if not host:
        faults += [fault(k + "_misaligned", k, {k: (lambda b, k=k, n=n: b.d.at(k, n))}, "d_%s must be" % w)
                   for k, n, w in (("flags", 2, "tile_flags"), ("linear", 4, "linear"), ("noise", 2, "noise"), ("support", 2, "support"), ("info", 2, "info"))]
        # 64 chunks of 2 samples (variant bits 3..4 = 2) where the workspace holds 62 planes of 1024 x 704: host arithmetic, before the context is looked at
        faults.append(fault("two_launches", "width", {"width": 1024, "height": 704, "spp": 128, "variant": 2 << 3}, solo=True))
    return _entry(name, context, good, body, faults, "null context")


def _select(name, context):
    host = name.endswith("_host")
    side = (lambda b: b.h) if host else (lambda b: b.d)
    good = {"below": lambda b: side(b).at("maps"), "above": lambda b: side(b).at("maps", 1024), "flags": lambda b: side(b).at("flags"), "sopts": True}

    def body(lib, rt, s):
        o = rt.TileSelectOpts(0.5, 2.0, 1, 0)
        tail = () if host else (None,)
        return getattr(lib, name)(s["ctx"], s["width"], s["height"], s["below"], s["above"], _ref(s["sopts"], o), s["flags"], *tail)

    size = "bad image size"
    faults = [fault(k + t, k, {k: v}, size) for k in ("width", "height") for t, v in (("_zero", 0), ("_negative", -3), ("_65537", BIG))]
    faults += [fault("null_maps", "below", {"below": None, "above": None}, "both null", solo=True), fault("null_flags", "flags", {"flags": None}, "d_tile_flags is null"),
               fault("null_opts", "sopts", {"sopts": False}, "opts is null"), fault("null_below_alone", "below", {"below": None}, solo=True)]
    faults += [fault(k + "_misaligned", k, {k: (lambda b, k=k, r=r, n=n: side(b).at(r, n))}, "d_%s must be" % w)
               for k, r, n, w in (("below", "maps", 2, "below_map"), ("above", "maps", 1026, "above_map"), ("flags", "flags", 2, "tile_flags"))]
    return _entry(name, context, good, body, faults, {"null": "null context", "empty": "accepted", "scene": "accepted"})


def _unpermute(context):
    good = {"n_ranks": 1, "gathered": lambda b: b.d.at("gathered"), "linear": lambda b: b.d.at("linear"), "rgb8": lambda b: b.d.at("rgb8")}

    def body(lib, rt, s):
        return lib.rtk_tiles_unpermute(s["ctx"], s["width"], s["height"], s["n_ranks"], s["real_mode"], s["gathered"], s["linear"], s["rgb8"], None)

    bad = "bad argument"
    faults = [fault(k + t, k, {k: v}, bad if v <= 0 else "", solo=v > 0) for k in ("width", "height") for t, v in (("_zero", 0), ("_negative", -3), ("_65537", BIG))]
    faults += [fault("n_ranks_zero", "n_ranks", {"n_ranks": 0}, bad), fault("null_gathered", "gathered", {"gathered": None}, bad),
               fault("real_mode_2", "real_mode", {"real_mode": 2}, solo=True), fault("real_mode_negative", "real_mode", {"real_mode": -1}, solo=True)]
    return _entry("rtk_tiles_unpermute", context, good, body, faults, {"null": bad, "empty": "accepted", "scene": "accepted"})


def _frame_launches(context):
    def body(lib, rt, s):
        return lib.rtk_frame_launches(_ref(s["cam"], _camera(rt, s)), _ref(s["opts"], _opts(rt, s)))

    bad = "bad camera or options"
    faults = [f._replace(names=bad) for f in NULLS] + _camera_faults(bad, depth_solo=True) + [
        fault("rank_0_of_0", "rank", {"rank": (0, 0)}, bad), fault("rank_negative", "rank", {"rank": (-1, 1)}, solo=True), fault("rank_1_of_1", "rank", {"rank": (1, 1)}, solo=True),
        fault("real_mode_2", "real_mode", {"real_mode": 2}, solo=True), fault("real_mode_negative", "real_mode", {"real_mode": -1}, solo=True)]
    return _entry("rtk_frame_launches", context, {}, body, faults, {k: "accepted" for k in KINDS}, writes=False)


def _progressive_create(context):
    def body(lib, rt, s):
        s["session"] = C.c_void_p()
        return lib.rtk_progressive_create(s["ctx"], _ref(s["cam"], _camera(rt, s)), _ref(s["opts"], _opts(rt, s)), _ref(s["out"], s["session"]))

    def after(lib, rt, s):
        lib.rtk_progressive_destroy(s["session"])

    faults = NULLS + [fault("null_out", "out", {"out": False}, "null argument")] + _camera_faults("bad camera dimensions") + _rank_faults("bad rank") + REAL_MODE
    return _entry("rtk_progressive_create", context, {"out": True}, body, faults, "null argument", after, writes=False)


def _multi_enqueue(context):
    """One device: the frame is rtk_render_device's, with the rank set by the call."""
    good = {"linear": lambda b: b.d.at("linear"), "rgb8": lambda b: b.d.at("rgb8")}

    def body(lib, rt, s):
        return lib.rtk_render_multi_enqueue(s["ctx"], _ref(s["cam"], _camera(rt, s)), _ref(s["opts"], _opts(rt, s)), s["linear"], s["rgb8"])

    def after(lib, rt, s):
        assert lib.rtk_multi_wait(s["ctx"]) == 0

    faults = NULLS + _camera_faults("bad camera dimensions") + REAL_MODE + [
        fault("count_work", "count_work", {"count_work": 1}, "work counters are per device"), fault("variant_bit_22", "variant", {"variant": BIT22}, "d_rgb8 must be null")]
    faults += [f._replace(solo=True, names="") for f in _rank_faults("")]
    return _entry("rtk_render_multi_enqueue", context, good, body, faults, "null argument", after)


def entries(context):
    """{name: Entry} of the 12 entry points for `context`."""
    made = [_render("rtk_render_device", context), _render("rtk_render_host", context), _views("rtk_render_views", context), _views("rtk_render_views_host", context),
            _render_tiles("rtk_render_tiles", context), _render_tiles("rtk_render_tiles_host", context), _select("rtk_tiles_select", context),
            _select("rtk_tiles_select_host", context), _unpermute(context), _frame_launches(context), _progressive_create(context), _multi_enqueue(context)]
    assert len(made) == 12
    return {e.name: e for e in made}


NO_CONTEXT = ("rtk_frame_launches",)               # besides the "null" column: what the CPU suite replays
