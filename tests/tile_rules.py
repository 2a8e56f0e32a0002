"""The rule of rtk_tiles_select (include/rtk.h, "Tile lists") restated in numpy, and the small helpers the tile-list tests share.
Data and functions only -- the tests are in test_tile_lists.py.

  raw flags   an in-image pixel q is raw-flagged when a below map is given and !(below_map[q] >= below), or an above map is
              given and !(above_map[q] <= above): a NaN flags, a value equal to its threshold does not, two maps are OR-ed.
              Maps and thresholds are float32, as on the device.
  dilation    tile t (8x8, row-major over the tiles, clipped to the image) is flagged iff a raw-flagged pixel lies within
              `dilate` of one of the tile's in-image pixels in both x and y.
"""
import numpy as np

TILE = 8


def tiles_of(width, height):
    return -(-width // TILE), -(-height // TILE)


def raw_flags(below_map=None, above_map=None, below=0.0, above=0.0):
    """(H, W) bool."""
    assert below_map is not None or above_map is not None
    raw = None
    with np.errstate(invalid="ignore"):
        if below_map is not None:
            raw = ~(np.asarray(below_map, np.float32) >= np.float32(below))
        if above_map is not None:
            a = ~(np.asarray(above_map, np.float32) <= np.float32(above))
            raw = a if raw is None else (raw | a)
    return raw


def dilate_to_tiles(raw, dilate):
    """Tile flags (int32, row-major over the tiles) of an (H, W) bool array of raw flags."""
    h, w = raw.shape
    tx, ty = tiles_of(w, h)
    flags = np.zeros(tx * ty, np.int32)
    for t in range(tx * ty):
        x0, y0 = (t % tx) * TILE, (t // tx) * TILE
        x1, y1 = min(x0 + TILE - 1, w - 1), min(y0 + TILE - 1, h - 1)   # the tile's in-image pixels
        window = raw[max(y0 - dilate, 0):min(y1 + dilate, h - 1) + 1, max(x0 - dilate, 0):min(x1 + dilate, w - 1) + 1]
        flags[t] = 1 if window.any() else 0
    return flags


def select(below_map=None, above_map=None, below=0.0, above=0.0, dilate=0):
    return dilate_to_tiles(raw_flags(below_map, above_map, below, above), dilate)


def pixel_mask(flags, width, height):
    """(H, W) bool: the in-image pixels of the tiles whose flag is non-zero."""
    tx, ty = tiles_of(width, height)
    m = (np.asarray(flags).reshape(ty, tx) != 0)
    return np.repeat(np.repeat(m, TILE, 0), TILE, 1)[:height, :width]


def flag_patterns(width, height, seed=7):
    """{name: flags} of the patterns the render tests use: none, all, only the last (corner) tile, a checkerboard, random 30 %."""
    tx, ty = tiles_of(width, height)
    n = tx * ty
    last = np.zeros(n, np.int32)
    last[-1] = 1
    checker = ((np.arange(n) % tx + np.arange(n) // tx) % 2).astype(np.int32)
    rnd = (np.random.default_rng(seed).random(n) < 0.3).astype(np.int32)
    rnd[int(np.random.default_rng(seed + 1).integers(n))] = 5      # any non-zero value flags; and the pattern is never empty
    return {"none": np.zeros(n, np.int32), "all": np.ones(n, np.int32), "last": last, "checker": checker, "random": rnd}
