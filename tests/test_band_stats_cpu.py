"""The band statistics as the library states them (csrc/band_hist.h, proj_roadsurf_amd/band_stats.py), the parts that need no GPU: the
host restatement ``rs_host_band_hist`` against the numpy route on seeded cases (tests/band_hist_cases.py), edge cells checked by hand,
``stats_from_hist`` against pandas on the pixel arrays themselves, ``reduce_band_hist`` / ``cover_stats`` against the histogram of the
concatenated pixels, the C ABI's new entries, their structure and their argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from proj_roadsurf_amd import band_stats as B
from proj_roadsurf_amd.engine import RsBandHist, load_library
from tests import band_hist_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rs_op_band_hist", "rs_host_band_hist", "rs_engine_fetch_band_hist_async", "rs_engine_fetch_band_hist_wait")


# ---------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", V.CPU_NAMES)
def test_host_restatement_equals_the_numpy_route(name):
    b = V.case(name)
    want = B.band_hist_host(b["tiles"], b["labels"])
    assert [w.shape for w in want] == [(len(labs), b["tiles"].shape[3], 256) for labs in b["labels"]] and want[0].dtype == np.uint32
    want = np.concatenate(want)
    got = B.band_hist_library_host(b["tiles"], b["packed"], b["tile_first"], prefill=0)
    again = B.band_hist_library_host(b["tiles"], b["packed"], b["tile_first"], prefill=7)      # whatever the buffer held: the entry clears it
    assert got.dtype == np.uint32 and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(again, want)
    assert want.sum() > 0
    assert np.array_equal(want.sum(axis=2), np.repeat(want.sum(axis=2)[:, :1], want.shape[1], axis=1))      # every band sees the same pixels


def test_shape_cases_hold_what_they_are_named_for():
    b = V.case("shapes_c3")
    h = B.band_hist_library_host(b["tiles"], b["packed"], b["tile_first"])
    nodata = int((~b["tiles"][0].any(axis=2)).sum())
    assert nodata >= 200 and int(h[0, 0].sum()) == 72 * 72 - nodata           # the full-tile label: every pixel but the nodata ones
    assert not h[1].any()                                                      # the empty label
    assert h[2].sum(axis=1).tolist() == [1, 1, 1]                              # one pixel: the last of the last row
    assert [int(np.flatnonzero(h[2, c])[0]) for c in range(3)] == b["tiles"][0, 71, 71].tolist()
    assert int(h[3, 0].sum()) > 7 * 28                                         # both rings count
    assert 0 < int(h[4, 0].sum()) <= 30 * 20 - 10 * 20                         # the nodata block inside the label is left out
    assert b["tile_first"].tolist() == [0, 5, 5, 6]
    assert h[5, 0, 7] == h[5, 1, 0] == h[5, 2, 200] == 72 * 72 and int(h[5].sum()) == 3 * 72 * 72      # uniform: one bin per band


def test_edge_cells_by_hand():
    """An 8 x 8 tile of 3 bands written by hand, canvases written bit by bit."""
    tile = np.zeros((1, 8, 8, 3), np.uint8)
    tile[0, 0, 0] = (0, 0, 0)              # nodata inside label 2
    tile[0, 0, 1] = (0, 9, 255)            # one zero band: counted, in bin 0 of band 0
    tile[0, 0, 2] = (255, 255, 255)
    tile[0, 7, 7] = (1, 2, 3)              # last column of the last row
    tile[0, 3, 7] = (4, 5, 6)              # last column
    tile[0, 7, 0] = (7, 8, 9)              # last row
    masks = np.zeros((4, 8, 8), bool)
    masks[1, 7, 7] = True                  # label 1: one pixel; label 0: none
    masks[2, 0, 0:3] = True                # label 2: the nodata pixel, the one-zero-band pixel, the 255 pixel
    masks[3, 3, 7] = masks[3, 7, 0] = masks[3, 7, 7] = True
    masks[3, 5, 5] = True                  # a nodata pixel again
    packed = np.packbits(masks, axis=2, bitorder="little")
    first = np.array([0, 4], np.int32)
    h = B.band_hist_library_host(tile, packed, first, prefill=99)
    assert np.array_equal(h, B.hist_of_rasters(tile, packed, first))
    assert not h[0].any()
    assert h[1].sum() == 3 and h[1, 0, 1] == h[1, 1, 2] == h[1, 2, 3] == 1
    assert h[2].sum() == 6 and h[2, 0, 0] == 1 and h[2, 0, 255] == 1 and h[2, 1, 9] == 1 and h[2, 1, 255] == 1 and h[2, 2, 255] == 2
    assert h[3].sum() == 9 and h[3, 0].nonzero()[0].tolist() == [1, 4, 7] and h[3, 2].nonzero()[0].tolist() == [3, 6, 9]


# ---------------------------------------------------------------------------------------------------- from histograms to columns
def _samples():
    """Pixel arrays of one band: tiny, even and odd counts, a constant, a narrow and a wide spread, a large one."""
    out = [np.array([17]), np.array([3, 250]), np.array([5, 5, 6]), np.full(1000, 42), np.array([0, 0, 255, 255])]
    for seed, n, lo, hi in ((1, 999, 0, 256), (2, 1000, 100, 110), (3, 50001, 0, 256), (4, 300000, 20, 240), (5, 4, 0, 256), (6, 77, 250, 256)):
        out.append(np.random.default_rng(seed).integers(lo, hi, n))
    return [a.astype(np.int64) for a in out]


def _far_from_a_rounding_boundary(x: float) -> bool:
    return abs(x * 100 - math.floor(x * 100) - 0.5) > 1e-9


def test_stats_from_hist_against_pandas():
    import pandas as pd
    worst = 0.0
    for px in _samples():
        got = B.stats_from_hist(np.bincount(px, minlength=256))[0]
        s = pd.Series(px)
        assert got["min"] == s.min() and got["max"] == s.max() and got["count"] == s.count() == len(px)
        assert got["median"] == s.median() and got["mean_exact"] == s.mean()
        assert _far_from_a_rounding_boundary(s.mean()) and got["mean"] == s.mean().round(2)
        if len(px) == 1:
            assert math.isnan(s.std()) and math.isnan(got["std_exact"]) and math.isnan(got["std"]) and math.isnan(got["margin"])
            continue
        std = float(s.std())
        rel = abs(got["std_exact"] - std) / std if std else abs(got["std_exact"])
        worst = max(worst, rel)
        print(f"n {len(px)}: std {got['std_exact']!r} pandas {std!r} relative difference {rel:.2e}")
        assert rel <= 1e-12
        margin = 2 * std / len(px) ** (1 / 2)
        assert _far_from_a_rounding_boundary(std) and _far_from_a_rounding_boundary(margin)
        assert got["std"] == np.round(std, 2) and got["margin"] == np.round(margin, 2)
    print(f"worst relative difference of the unrounded std: {worst:.2e}")


def test_stats_against_a_pandas_frame_grouped_as_the_reference_groups():
    """One row per pixel, grouped by road: the aggregation of the reference's table, written with pandas' own functions."""
    import pandas as pd
    rng = np.random.default_rng(11)
    roads = {"a": rng.integers(0, 256, 4000), "b": rng.integers(90, 140, 1501), "c": rng.integers(0, 3, 2)}
    frame = pd.DataFrame({"road": np.repeat(list(roads), [len(v) for v in roads.values()]), "value": np.concatenate(list(roads.values()))})
    table = frame.groupby("road")["value"].agg(["min", "max", "median", "mean", "count", "std"])
    table["margin"] = 2 * table["std"] / table["count"] ** (1 / 2)
    for rid, px in roads.items():
        got = B.stats_from_hist(np.bincount(px, minlength=256))[0]
        row = table.loc[rid]
        assert (got["min"], got["max"], got["median"], got["mean_exact"], got["count"]) == (row["min"], row["max"], row["median"], row["mean"], row["count"])
        assert abs(got["std_exact"] - row["std"]) <= 1e-12 * row["std"]
        assert all(_far_from_a_rounding_boundary(float(row[k])) for k in ("mean", "std", "margin"))
        assert (got["mean"], got["std"], got["margin"]) == (round(row["mean"], 2), np.round(row["std"], 2), np.round(row["margin"], 2))


def test_an_empty_band_and_the_shapes_taken():
    rows = B.stats_from_hist(np.zeros((2, 256), np.uint32))
    assert len(rows) == 2 and rows[0]["count"] == 0 and all(math.isnan(rows[0][k]) for k in ("min", "max", "median", "mean", "std", "margin"))
    assert B.json_rows(rows)[0]["min"] is None and B.json_rows(rows)[0]["count"] == 0
    assert set(B.COLUMNS) <= set(rows[0])
    with pytest.raises(ValueError):
        B.stats_from_hist(np.zeros((2, 255)))


# ---------------------------------------------------------------------------------------------------- from tiles to roads
def _pixels_under(tile, packed_label):
    side = tile.shape[0]
    bits = np.unpackbits(packed_label, axis=1, bitorder="little")[:, :side].astype(bool)
    return tile[bits & tile.any(axis=2)]


def test_reduce_and_cover_stats_equal_the_histogram_of_the_concatenated_pixels():
    b = V.case("side72_c3")
    tables = B.band_hist_host(b["tiles"], b["labels"])
    ids = [["r0", "r1", "r2"], ["r1", "r3", "r0", "r4", "r1", "r5"]]            # r0 and r1 have pieces in both tiles, r1 two in one
    by_road = B.reduce_band_hist(tables, ids)
    assert list(by_road) == ["r0", "r1", "r2", "r3", "r4", "r5"]
    px = {}
    g = 0
    for t, row in enumerate(ids):
        for rid in row:
            px.setdefault(rid, []).append(_pixels_under(b["tiles"][t], b["packed"][g]))
            g += 1
    for rid, parts in px.items():
        allpx = np.concatenate(parts)
        want = np.stack([np.bincount(allpx[:, c], minlength=256) for c in range(3)])
        assert by_road[rid].dtype == np.int64 and np.array_equal(by_road[rid], want), rid
    back = B.reduce_band_hist(tables[::-1], ids[::-1])                         # the order of the tiles does not matter
    assert all(np.array_equal(back[r], by_road[r]) for r in by_road)
    cover = {"r0": "artificial", "r1": "natural", "r2": "artificial", "r3": "natural", "r4": None}       # r5: no entry
    got = B.cover_stats(by_road, cover)
    assert list(got) == ["artificial", "natural"]
    for name, members in (("artificial", ("r0", "r2")), ("natural", ("r1", "r3"))):
        allpx = np.concatenate([p for r in members for p in px[r]])
        want = B.stats_from_hist(np.stack([np.bincount(allpx[:, c], minlength=256) for c in range(3)]))
        assert got[name] == want and got[name][0]["count"] == len(allpx) > 0
    assert B.cover_stats(back, cover) == got
    assert B.reduce_band_hist([], []) == {}
    with pytest.raises(ValueError):
        B.reduce_band_hist(tables, ids[:1])


# ---------------------------------------------------------------------------------------------------- ABI
def test_header_library_and_ctypes_agree():
    hdr = open(os.path.join(ROOT, "include", "rs_engine.h")).read()
    lib = load_library()
    for name in ENTRIES:
        assert f"int {name}(" in hdr, name
        assert hasattr(lib, name), name
    body = re.search(r"typedef struct rs_band_hist \{(.*?)\} rs_band_hist;", hdr, re.S).group(1)
    fields = re.findall(r"(uint32_t)\*\s+(\w+);", body)
    assert [(n, C.POINTER(C.c_uint32)) for _, n in fields] == list(RsBandHist._fields_)
    assert C.sizeof(RsBandHist) == C.sizeof(C.c_void_p)
    for name, count in (("rs_op_band_hist", 9), ("rs_host_band_hist", 8), ("rs_engine_fetch_band_hist_async", 8), ("rs_engine_fetch_band_hist_wait", 1)):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == count == len(getattr(lib, name).argtypes), name
    src = open(os.path.join(ROOT, "proj_roadsurf_amd", "csrc", "band_hist.h")).read()
    assert "#define BH_MAX_SIDE 1024" in src and "#define BH_MAX_CHANNELS 4" in src and "#define BH_BINS 256" in src
    assert lib.rs_abi_version() == 1


def test_entries_refuse_bad_arguments_before_touching_anything():
    """No GPU here and the pointers are not memory: a call that got past its checks would fault or fail with a HIP error."""
    lib = load_library()
    err = lambda: lib.rs_last_error().decode()
    one = C.c_void_p(256)
    good = [one, one, one, 1, 1, 32, 3, one]
    for fn, tail in ((lib.rs_op_band_hist, [None]), (lib.rs_host_band_hist, [])):
        name = "rs_op_band_hist" if tail else "rs_host_band_hist"
        for i in (0, 1, 2, 7):
            bad = list(good)
            bad[i] = None
            assert fn(*bad, *tail) == -1 and "null" in err() and name in err(), (name, i, err())
        for i, values, word, code in ((3, (0, -1), "n_tiles", -1), (4, (-1,), "n_inst", -1), (5, (0, -8, 1025, 1032), "side", -1),
                                      (6, (0, -1, 5), "channels", -1), (5, (1, 5, 9, 13), "multiple of 4", -4)):
            for v in values:
                bad = list(good)
                bad[i] = v
                assert fn(*bad, *tail) == code and name in err() and word in err(), (name, i, v, err())
    assert lib.rs_engine_fetch_band_hist_async(None, 1, None, None, None, None, None, None) < 0 and "rs_engine_fetch_band_hist_async" in err()
    assert lib.rs_engine_fetch_band_hist_wait(None) < 0
