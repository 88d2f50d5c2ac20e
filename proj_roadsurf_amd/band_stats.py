"""The statistical route to a road's cover (R:scripts/statistical_analysis/statistical_analysis.py with ``fct_misc.get_pixel_values``
and ``fct_statistics.get_df_stats_groupby`` / ``get_df_stats_no_group``): per road and band the min, max, median, mean, std and count
of the pixels under the road's polygon, over all tiles the road touches, without the nodata pixels -- and the same per cover type.

The reference loops over roads x tiles with ``rasterio.mask`` and keeps one pandas row per pixel.  Here the pixels are never listed:
every column is an exact function of a 256-bin histogram per (road, band), and integer histograms add exactly over tiles, batches and
ranks.  csrc/band_hist.h states the counting rule (a pixel counts where the label's canvas bit is set and not all bands are 0);
``band_hist_kernel`` runs it on the device behind the forward (``Engine.band_hist``, ``LanePipeline.run(..., band_stats=True)``),
``rs_host_band_hist`` restates it as plain loops, and ``band_hist_host`` is the numpy route: the fallback of a batch that does not fit
the device pool, and the yardstick of the tests.

Differences from the reference, by construction: a road's pixels are whole pixels of the tile grid whose centres lie inside the label
(the rasteriser of the training targets, not rasterio's ``all_touched`` choice), and there is a single nodata rule -- every band 0 --
where the reference first asks the TIFF for a nodata value.  Per-pixel band ratios, VgNIR-BI, PCA, KS tests and plots are not
restated; the histograms carry what a later KS statistic needs."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Dict, Hashable, List, Optional, Sequence

import numpy as np

BINS = 256
COLUMNS = ("min", "max", "median", "mean", "count", "std", "margin")      # get_df_stats_groupby's, in its order


def hist_of_rasters(tiles: np.ndarray, packed: np.ndarray, tile_first: np.ndarray) -> np.ndarray:
    """The rule of csrc/band_hist.h in numpy: tiles (n, side, side, C) uint8, packed (n_inst, side, ceil(side / 8)) bit-packed label
    canvases, tile_first (n + 1,) -> hist (n_inst, C, 256) uint32."""
    n, side, _, ch = tiles.shape
    out = np.zeros((int(packed.shape[0]), ch, BINS), np.uint32)
    for t in range(n):
        data = tiles[t].any(axis=2)
        for g in range(int(tile_first[t]), int(tile_first[t + 1])):
            bits = np.unpackbits(packed[g], axis=1, bitorder="little")[:, :side].astype(bool)
            px = tiles[t][bits & data]
            for c in range(ch):
                out[g, c] = np.bincount(px[:, c], minlength=BINS)
    return out


def band_hist_host(tiles: np.ndarray, labels: Sequence[Sequence[Sequence[np.ndarray]]]) -> List[np.ndarray]:
    """The numpy route to what ``Engine.band_hist`` gives: tiles (n, side, side, C) uint8, labels[tile][label] = list of rings ([x0, y0,
    ...], tile pixels) -> per tile an (L_t, C, 256) uint32 array.  ``raster_vote.label_rasters`` and ``np.bincount``."""
    from .raster_vote import label_rasters
    tiles = np.asarray(tiles)
    if tiles.ndim != 4 or tiles.dtype != np.uint8 or len(labels) != tiles.shape[0]:
        raise ValueError(f"{len(labels)} label lists for tiles {tiles.dtype} {tiles.shape}")
    out = []
    for t, labs in enumerate(labels):
        packed = label_rasters(labs, tiles.shape[1], tiles.shape[2])
        out.append(hist_of_rasters(tiles[t:t + 1], packed, np.array([0, len(labs)])))
    return out


def _hist_call(entry: str, tiles: np.ndarray, packed: np.ndarray, tile_first: np.ndarray, prefill: int, device: bool) -> np.ndarray:
    from .engine import _check, load_library
    lib = load_library()
    tiles = np.ascontiguousarray(tiles, np.uint8)
    n, side, _, ch = tiles.shape
    packed = np.ascontiguousarray(packed, np.uint8)
    first = np.ascontiguousarray(tile_first, np.int32)
    n_inst = int(packed.shape[0])
    hist = np.full((n_inst, ch, BINS), prefill, np.uint32)
    if not device:
        _check(lib, lib.rs_host_band_hist(tiles.ctypes.data, packed.ctypes.data if n_inst else None, first.ctypes.data, n, n_inst, side, ch,
                                          hist.ctypes.data if n_inst else None), entry)
        return hist
    import torch
    dev = [torch.from_numpy(a.view(np.uint8) if a.dtype == np.uint32 else a).cuda() for a in (tiles, packed, first, hist)]
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_band_hist(dev[0].data_ptr(), dev[1].data_ptr() if n_inst else None, dev[2].data_ptr(), n, n_inst, side, ch,
                                    dev[3].data_ptr() if n_inst else None, None), entry)
    torch.cuda.synchronize()
    return dev[3].cpu().numpy().view(np.uint32).reshape(n_inst, ch, BINS)


def band_hist_library_host(tiles: np.ndarray, packed: np.ndarray, tile_first: np.ndarray, prefill: int = 0) -> np.ndarray:
    """``rs_host_band_hist`` on tiles (n, side, side, C), packed canvases (n_inst, side, ceil(side / 8)) and tile_first (n + 1,) -> hist
    (n_inst, C, 256) uint32.  ``prefill``: what the output holds before the call (the entry clears it itself).  Needs no device."""
    return _hist_call("rs_host_band_hist", tiles, packed, tile_first, prefill, False)


def band_hist_device(tiles: np.ndarray, packed: np.ndarray, tile_first: np.ndarray, prefill: int = 0) -> np.ndarray:
    """``rs_op_band_hist`` on the same arrays, uploaded through torch: the kernel's table."""
    return _hist_call("rs_op_band_hist", tiles, packed, tile_first, prefill, True)


def reduce_band_hist(tables: Sequence[np.ndarray], road_ids: Sequence[Sequence[Hashable]]) -> Dict[Hashable, np.ndarray]:
    """From the per-(tile, label) histograms to one per road: tables[tile] = (L_t, C, 256) as ``Engine.band_hist`` / ``band_hist_host``
    give them, road_ids[tile] = the road of each of the tile's labels.  A road's pieces -- its labels over all tiles -- are summed in
    int64 (``np.add.at``); integer sums do not depend on the order of the tiles.  Roads come in order of first appearance."""
    if len(tables) != len(road_ids):
        raise ValueError(f"{len(road_ids)} road id lists for {len(tables)} tiles")
    index: Dict[Hashable, int] = {}
    rows: List[int] = []
    parts = []
    for t, ids in zip(tables, road_ids):
        t = np.asarray(t)
        if t.ndim != 3 or t.shape[0] != len(ids) or t.shape[2] != BINS:
            raise ValueError(f"a tile's histograms must be ({len(ids)}, C, {BINS}), got {t.shape}")
        rows.extend(index.setdefault(rid, len(index)) for rid in ids)
        if len(ids):
            parts.append(t.astype(np.int64))
    if not parts:
        return {}
    total = np.zeros((len(index),) + parts[0].shape[1:], np.int64)
    np.add.at(total, np.asarray(rows, np.int64), np.concatenate(parts))
    return {rid: total[r] for rid, r in index.items()}


def _band_columns(h: np.ndarray) -> Dict[str, float]:
    counts = [int(x) for x in h]
    n = sum(counts)
    nan = float("nan")
    if n == 0:
        return {"min": nan, "max": nan, "median": nan, "mean_exact": nan, "mean": nan, "count": 0, "std_exact": nan, "std": nan, "margin": nan}
    nz = [v for v, k in enumerate(counts) if k]
    # the two middle order statistics (0-based ranks (n - 1) // 2 and n // 2) off the cumulative counts
    cum = np.cumsum(h.astype(np.int64))
    lo, hi = int(np.searchsorted(cum, (n - 1) // 2 + 1)), int(np.searchsorted(cum, n // 2 + 1))
    s1 = sum(v * k for v, k in enumerate(counts))
    s2 = sum(v * v * k for v, k in enumerate(counts))
    mean = s1 / n                                       # int / int: correctly rounded
    if n > 1:
        std = math.sqrt(float(Fraction(n * s2 - s1 * s1, n * (n - 1))))        # ddof 1, from exact integer moments
        margin = float(np.round(2 * std / n ** (1 / 2), 2))                    # from the unrounded std, as get_df_stats_groupby
    else:
        std = margin = nan
    return {"min": nz[0], "max": nz[-1], "median": (lo + hi) / 2, "mean_exact": mean, "mean": float(np.round(mean, 2)), "count": n,
            "std_exact": std, "std": float(np.round(std, 2)), "margin": margin}


def stats_from_hist(h: np.ndarray) -> List[Dict[str, float]]:
    """The reference's columns per band from a (C, 256) histogram (a (256,) one is one band): ``min``, ``max``, ``count`` read off the
    counts; ``median`` the mean of the two middle order statistics; ``mean_exact`` the exact integer sum over the count in float64 and
    ``mean`` that rounded to 2 decimals; ``std_exact`` with ddof 1 from exact integer moments, (n * sum v^2 - (sum v)^2) / (n (n - 1))
    as a ``Fraction``, converted to float once, then the square root (NaN for a count of 1), ``std`` that rounded to 2 decimals;
    ``margin`` = round(2 * std_exact / sqrt(count), 2).  A band without pixels gives count 0 and NaN elsewhere.  Rounding is
    ``np.round``, as pandas' ``.round(2)``."""
    h = np.asarray(h)
    if h.ndim == 1:
        h = h[None]
    if h.ndim != 2 or h.shape[1] != BINS:
        raise ValueError(f"a histogram must be (C, {BINS}), got {h.shape}")
    return [_band_columns(h[c]) for c in range(h.shape[0])]


def cover_stats(hist_by_road: Dict[Hashable, np.ndarray], cover_of_road: Dict[Hashable, Hashable]) -> Dict[Hashable, List[Dict[str, float]]]:
    """The same columns per cover type: the histograms of the roads of every cover summed (int64), then ``stats_from_hist``.  Roads
    without an entry in ``cover_of_road`` (or with ``None``) enter no cover.  Covers come in order of first appearance."""
    total: Dict[Hashable, np.ndarray] = {}
    for rid, h in hist_by_road.items():
        cover = cover_of_road.get(rid)
        if cover is None:
            continue
        h = np.asarray(h).astype(np.int64)
        total[cover] = total[cover] + h if cover in total else h.copy()
    return {cover: stats_from_hist(h) for cover, h in total.items()}


def json_rows(stats: List[Dict[str, float]]) -> List[Dict[str, Optional[float]]]:
    """``stats_from_hist``'s rows for a JSON file: NaN becomes null."""
    return [{k: (None if isinstance(v, float) and math.isnan(v) else v) for k, v in row.items()} for row in stats]
