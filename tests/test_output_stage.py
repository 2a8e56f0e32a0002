"""Known answers for the output stage (-m gpu): rtk_unpermute_kernel and rtk_resolve_kernel share write_pixel / to_byte
(csrc/rtk_frame.hip, csrc/rtk_device_math.h), and every value they had seen so far came out of a render.  rtk_tiles_unpermute
takes a caller-made buffer, so here it is driven with chosen values: the thresholds of every byte and their neighbours one and
two units in the last place away, the clamp's edge, zeros, denormals, negatives, huge values, infinities and NaN.

Reference (numpy float64; the reference's image writer, Camera.txt:29-34,77-89):
    g = sqrt(x) if x > 0 else 0;  g = min(max(g, 0), 0.999);  byte = int(255.999 * g)
np.sqrt is correctly rounded, so the bytes must be EQUAL: a device square root that is not correctly rounded moves a threshold
value into the neighbouring byte and shows up here.  The F32 kernels widen the float to double first (to_byte(double(x))), so
the same rule applies to the float32 value.  The linear output is a copy: the input bit for bit (a NaN stays that NaN).

Shapes: images that are one pixel, one tile, ragged in both directions, with rank counts that leave padding tiles behind a
rank's last tile.  Slots of the gathered buffer that are no pixel of the image (the rest of an edge tile, padding tiles) hold
values whose bytes differ from the neighbouring pixel's by 128; the outputs lie between poisoned guard bands."""
import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.scene_cases import SCENE_SEED, scene_file

SHAPES = [(1, 1), (8, 8), (13, 7), (65, 9), (100, 60)]
RANKS = [1, 2, 3, 5, 8]
GUARD = 256                      # elements of poison before and after each output
FLT_MAX = float(np.finfo(np.float32).max)


def to_byte(x):
    """The reference's rule on float64 values, element-wise."""
    x = np.asarray(x, np.float64)
    pos = x > 0
    with np.errstate(invalid="ignore"):
        g = np.where(pos, np.sqrt(np.where(pos, x, 0.0)), 0.0)
    g = np.minimum(np.maximum(g, 0.0), 0.999)
    return (255.999 * g).astype(np.int64).astype(np.uint8)


def known_values(dtype):
    """Every byte's threshold (k / 255.999)^2 and the clamp's edge 0.999^2 with their neighbours at +-1 and +-2 ulp of
    `dtype`, then the special values."""
    dtype = np.dtype(dtype)
    centres = np.array([(k / 255.999) ** 2 for k in range(257)] + [0.999 ** 2]).astype(dtype)
    out = []
    for c in centres:
        lo1 = np.nextafter(c, dtype.type(-np.inf))
        hi1 = np.nextafter(c, dtype.type(np.inf))
        out += [np.nextafter(lo1, dtype.type(-np.inf)), lo1, c, hi1, np.nextafter(hi1, dtype.type(np.inf))]
    info = np.finfo(dtype)
    special = [0.0, -0.0, info.smallest_subnormal, -1.0, -info.tiny, -info.smallest_subnormal, 1.0, FLT_MAX, np.inf, -np.inf, np.nan]
    if dtype == np.float64:
        special.append(1e300)
    with np.errstate(over="ignore"):
        return np.concatenate([np.array(out, dtype), np.array(special, dtype)])


def test_reference_rule_on_hand_values():
    assert to_byte([0.0, -0.0, -1.0, np.nan, -np.inf]).tolist() == [0, 0, 0, 0, 0]
    assert to_byte([1.0, 1e300, np.inf, 0.999 ** 2 * 1.01]).tolist() == [255, 255, 255, 255]
    assert to_byte([0.25, 0.0625]).tolist() == [127, 63]          # int(255.999 * 0.5), int(255.999 * 0.25)
    v = known_values(np.float64)
    assert len(v) == 258 * 5 + 12 and len(known_values(np.float32)) == 258 * 5 + 11
    assert len(set(to_byte(v).tolist())) == 256                    # every byte value occurs


def gathered_from_image(img, n_ranks, offset):
    """The [n_ranks][tiles_per_rank][3][64] buffer a gather of the ranks' compact buffers gives for `img` (H, W, 3).  Slots that
    are no pixel of the image hold a value whose byte is the nearest pixel's + 128 (mod 256)."""
    h, w = img.shape[:2]
    tx, ty = (w + 7) // 8, (h + 7) // 8
    tpr = (tx * ty + n_ranks - 1) // n_ranks
    slot = np.arange(n_ranks * tpr)
    rank, local = slot // tpr, slot % tpr
    tile = local * n_ranks + rank                                  # include/rtk.h: tile t is rank t % n's local tile t / n
    pix = np.arange(64)
    x = (tile % tx)[:, None] * 8 + (pix & 7)[None, :]
    y = (tile // tx)[:, None] * 8 + (pix >> 3)[None, :]
    inside = (tile < tx * ty)[:, None] & (x < w) & (y < h)
    near = img[np.minimum(y, h - 1), np.minimum(x, w - 1)]         # [slots, 64, 3]
    pad_byte = (to_byte(near).astype(np.int64) + 128 + offset) % 256
    pad = (((pad_byte + 0.5) / 255.999) ** 2).astype(img.dtype)
    assert (to_byte(pad) == pad_byte).all()
    values = np.where(inside[:, :, None], near, pad)
    return np.ascontiguousarray(values.transpose(0, 2, 1)).reshape(n_ranks, tpr, 3, 64), int(inside.sum())


def _guarded(torch, n, dtype, poison, dev):
    buf = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


@pytest.mark.gpu
@pytest.mark.parametrize("real", ["f64", "f32"])
def test_unpermute_bytes_follow_the_reference_rule_and_linear_is_a_copy(rt, renderer, real):
    import torch

    dev = torch.device("cuda", renderer.device)
    mode, np_t, t_t, bits = (rt.RTK_REAL_F64, np.float64, torch.float64, np.uint64) if real == "f64" else (rt.RTK_REAL_F32, np.float32, torch.float32, np.uint32)
    values = known_values(np_t)
    seen = np.zeros(len(values), bool)
    case = 0
    for w, h in SHAPES:
        for n_ranks in RANKS:
            # every pixel channel takes the next known value; small images start at different places of the list
            start = (case * 211) % len(values)
            index = (start + np.arange(h * w * 3)) % len(values)
            seen[index] = True
            img = values[index].reshape(h, w, 3)
            gathered, n_inside = gathered_from_image(img, n_ranks, case)
            assert n_inside == w * h
            d_gathered = torch.from_numpy(gathered).to(dev)
            lin_all, lin = _guarded(torch, h * w * 3, t_t, -12345.0, dev)
            b8_all, b8 = _guarded(torch, h * w * 3, torch.uint8, 0xA5, dev)
            renderer.unpermute(w, h, n_ranks, mode, d_gathered.data_ptr(), lin.data_ptr(), b8.data_ptr())
            torch.cuda.synchronize()
            got_lin, got8 = lin.cpu().numpy().reshape(h, w, 3), b8.cpu().numpy().reshape(h, w, 3)
            where = (real, w, h, n_ranks)
            assert np.array_equal(got_lin.view(bits), img.view(bits)), where        # a copy, NaN payload included
            want8 = to_byte(img)
            bad = np.argwhere(got8 != want8)
            assert len(bad) == 0, (where, [(float(img[tuple(k)]).hex(), int(got8[tuple(k)]), int(want8[tuple(k)])) for k in bad[:8]])
            for all_, poison in ((lin_all, -12345.0), (b8_all, 0xA5)):
                edge = torch.cat([all_[:GUARD], all_[-GUARD:]]).cpu().numpy()
                assert (edge == poison).all(), where
            # each output alone: the other pointer null
            lin.fill_(-12345.0)
            b8.fill_(0xA5)
            renderer.unpermute(w, h, n_ranks, mode, d_gathered.data_ptr(), lin.data_ptr(), 0)
            torch.cuda.synchronize()
            assert np.array_equal(lin.cpu().numpy().reshape(h, w, 3).view(bits), img.view(bits)) and (b8_all == 0xA5).all().item(), where
            renderer.unpermute(w, h, n_ranks, mode, d_gathered.data_ptr(), 0, b8.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(b8.cpu().numpy().reshape(h, w, 3), want8), where
            case += 1
    assert seen.all()                                              # every known value went through the kernel


@pytest.mark.gpu
@pytest.mark.parametrize("real", ["f64", "f32"])
def test_rendered_bytes_follow_the_same_rule_from_their_own_linear_output(rt, renderer, real):
    """The resolve kernel on a frame with pixels above 1 (the Cornell box's light, seen directly) and at exactly 0 (paths that
    never reach it under a black background): its bytes are the numpy rule applied to its own linear output."""
    import torch

    scene = rt.Scene.build("cornell_box", SCENE_SEED, scene_file("cornell_box", GOLDEN))
    renderer.upload(scene)
    w, h = 67, 61
    cam = scene.camera(w, h, 2, 4)
    dev = torch.device("cuda", renderer.device)
    mode, t_t = (rt.RTK_REAL_F64, torch.float64) if real == "f64" else (rt.RTK_REAL_F32, torch.float32)
    lin_all, lin = _guarded(torch, h * w * 3, t_t, -12345.0, dev)
    b8_all, b8 = _guarded(torch, h * w * 3, torch.uint8, 0xA5, dev)
    renderer.render_device(cam, lin.data_ptr(), b8.data_ptr(), real_mode=mode, seed=3)
    torch.cuda.synchronize()
    got = lin.cpu().numpy().astype(np.float64)
    assert (got > 1.0).any() and (got == 0.0).any() and ((got > 0.0) & (got < 1.0)).any()
    assert np.array_equal(b8.cpu().numpy(), to_byte(got))
    for all_, poison in ((lin_all, -12345.0), (b8_all, 0xA5)):
        assert (torch.cat([all_[:GUARD], all_[-GUARD:]]).cpu().numpy() == poison).all()
