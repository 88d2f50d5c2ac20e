"""Seeded, small cases for the band histograms (csrc/band_hist.h), shared by tests/test_band_stats_cpu.py and
tests/test_gpu_band_stats.py.  A case is a dict: ``tiles`` (n, side, side, C) uint8, ``labels`` [tile][label] = list of rings in tile
pixels, ``packed`` (n_inst, side, ceil(side / 8)) the labels' canvases (``raster_vote.label_rasters``), ``tile_first`` (n + 1,) int32."""
import functools

import numpy as np

from proj_roadsurf_amd.raster_vote import label_rasters


def rect(x0, y0, x1, y1):
    return np.array([x0, y0, x1, y0, x1, y1, x0, y1], np.float64)


def _road(rng, side):
    """A road-shaped label: a thick segment between two points of the tile's border region, as a quadrilateral."""
    a, b = rng.uniform(-2, side + 2, 2), rng.uniform(-2, side + 2, 2)
    d = b - a
    norm = np.hypot(*d)
    nrm = np.array([-d[1], d[0]]) / (norm if norm > 0 else 1.0) * rng.uniform(0.6, max(1.0, side / 10))
    return np.concatenate([a + nrm, b + nrm, b - nrm, a - nrm]).astype(np.float64)


def _tiles(rng, n, side, ch, nodata=0.05):
    """Random tiles with runs of every kind of pixel the rule tells apart: nodata (every band 0), one band 0, value 255."""
    t = rng.integers(0, 256, (n, side, side, ch), dtype=np.uint8)
    kind = rng.random((n, side, side))
    t[kind < nodata] = 0
    one = (kind >= nodata) & (kind < 2 * nodata)
    t[..., 0][one] = 0
    t[..., ch - 1][(kind >= 2 * nodata) & (kind < 3 * nodata)] = 255
    t[:, -1, :, :] = np.maximum(t[:, -1, :, :], 1)          # the last row and the last column hold data
    t[:, :, -1, :] = np.maximum(t[:, :, -1, :], 1)
    return t


def _pack(tiles, labels):
    side = tiles.shape[1]
    packed = np.concatenate([label_rasters(labs, side, side) for labs in labels] + [np.zeros((0, side, (side + 7) // 8), np.uint8)])
    first = np.concatenate([[0], np.cumsum([len(labs) for labs in labels])]).astype(np.int32)
    return {"tiles": tiles, "labels": labels, "packed": np.ascontiguousarray(packed), "tile_first": first}


def _random(seed, n, side, ch, per_tile):
    rng = np.random.default_rng(seed)
    tiles = _tiles(rng, n, side, ch)
    labels = []
    for k in per_tile:
        labs = [[_road(rng, side)] for _ in range(k)]
        if k:
            labs[0] = [rect(side - 3.0, 0.0, float(side), float(side))]                  # the last columns, every row
        if k > 1:
            labs[1] = [rect(0.0, side - 2.0, float(side), float(side))]                  # the last rows, every column
        labels.append(labs)
    return _pack(tiles, labels)


# the sizes: 32 (rows of one word), 40 (rows of 5 bytes: words straddle rows), 72 (rows of 9 bytes), 128 (one chunk of 512 words),
# 264 (2 178 words: two workgroups per label, the second partly past the canvas), 1024 (16 workgroups per label)
@functools.lru_cache(maxsize=None)
def case(name):
    if name == "side32_c3":
        return _random(32, 3, 32, 3, (4, 0, 3))             # a tile without labels between two tiles with labels
    if name == "side40_c4":
        return _random(40, 2, 40, 4, (5, 2))
    if name == "side72_c3":
        return _random(72, 2, 72, 3, (3, 6))
    if name == "side128_c4":
        return _random(128, 2, 128, 4, (6, 1))
    if name == "side264_c3":
        return _random(264, 1, 264, 3, (4,))
    if name == "shapes_c3":
        # side 72: a full-tile label, an empty label (no pixel centre inside), a one-pixel label, a label of two rings, a label over
        # a block of nodata pixels; then a tile without labels; then a uniform tile under a full-tile label (every pixel in one bin)
        rng = np.random.default_rng(7)
        tiles = _tiles(rng, 3, 72, 3)
        tiles[0, 10:20, 30:50] = 0
        tiles[2] = np.array([7, 0, 200], np.uint8)
        full = [rect(0.0, 0.0, 72.0, 72.0)]
        labels = [[full, [rect(3.1, 3.1, 3.4, 3.4)], [rect(71.0, 71.0, 72.0, 72.0)], [rect(2.0, 2.0, 9.0, 30.5), rect(40.5, 50.0, 70.0, 72.0)],
                   [rect(25.0, 5.0, 55.0, 25.0)]], [], [full]]
        return _pack(tiles, labels)
    if name == "shapes_c4":
        rng = np.random.default_rng(8)
        tiles = _tiles(rng, 2, 40, 4)
        tiles[1] = np.array([255, 255, 1, 0], np.uint8)
        full = [rect(0.0, 0.0, 40.0, 40.0)]
        return _pack(tiles, [[full, [rect(0.0, 0.0, 1.0, 1.0)], [rect(50.0, 50.0, 60.0, 60.0)]], [full, [rect(39.0, 0.0, 40.0, 40.0)]]])
    if name == "labels128_c3":
        rng = np.random.default_rng(9)
        tiles = _tiles(rng, 2, 32, 3)
        return _pack(tiles, [[[_road(rng, 32)] for _ in range(128)], [[rect(0.0, 0.0, 32.0, 32.0)]]])
    if name == "side1024_c4":
        rng = np.random.default_rng(10)
        tiles = _tiles(rng, 1, 1024, 4, nodata=0.01)
        return _pack(tiles, [[[rect(0.0, 0.0, 1024.0, 1024.0)]]])
    raise KeyError(name)


CPU_NAMES = ("side32_c3", "side40_c4", "side72_c3", "side128_c4", "side264_c3", "shapes_c3", "shapes_c4", "labels128_c3")
GPU_NAMES = CPU_NAMES + ("side1024_c4",)
