"""The polygon geometry of the road vote on the host (csrc/poly_overlap.h, rs_host_polygon_overlaps, rs_host_road_votes_area_sweep):
the exact checker pinned by hand areas and pixel counts, the two conditions that keep the bars honest, the host restatement against
the checker within po_bound, every weight against the rounding of the exact quotient, the sweep's slices, the pixel tables on
rectilinear shapes, the refusals and reduce_votes on float64 areas.  Needs the built library, no device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import poly_overlap_ref as ref
from tests import poly_vote_cases as pc
from proj_roadsurf_amd import raster_vote as rv
from proj_roadsurf_amd.engine import RsError, load_library

NAMES = [c["name"] for c in pc.cases()]
SWEEPS = {1: [0.3], 20: [float(t) for t in np.arange(0, 1., 0.05)], 32: [float(t) for t in np.linspace(0.97, 0.0, 32)]}


# ---------------------------------------------------------------------------------------------------- the checker
@pytest.mark.parametrize("i", range(len(ref.HAND)))
def test_checker_hand_areas(i):
    P, Q, want = ref.HAND[i]
    assert ref.intersection_area(P, Q) == want
    assert ref.intersection_area(Q, P) == want
    assert ref.intersection_area([r[::-1] for r in P], Q) == want


def test_checker_pixel_counts():
    """Integer rectilinear polygons: the area of the intersection is the popcount of the AND of their rasters."""
    side = 32
    shapes = [[pc.rect(3, 4, 20, 17)], [pc.L_SHAPE], [pc.comb(1, 2, 24, 5, 10)], [pc.rect(2, 2, 30, 30), pc.rect(10, 10, 22, 22)],
              [pc.rect(0, 0, 7, 32), pc.rect(9, 20, 31, 29)]]
    flat = [[np.array([float(v) for p in ring for v in p]) for ring in s] for s in shapes]
    # label_rasters ORs a label's rings; a hole is the XOR of the two rasters
    ras = []
    for s, f in zip(shapes, flat):
        bits = [np.unpackbits(rv.label_rasters([[r]], side, side)[0], axis=1, bitorder="little")[:, :side].astype(bool) for r in f]
        m = bits[0]
        for b in bits[1:]:
            m = m ^ b
        ras.append(m)
        assert int(m.sum()) == ref.intersection_area(s, [pc.rect(0, 0, side, side)])
    for i in range(len(shapes)):
        for j in range(len(shapes)):
            assert ref.intersection_area(shapes[i], shapes[j]) == int((ras[i] & ras[j]).sum()), (i, j)


def test_checker_agrees_with_the_rule_in_exact_arithmetic():
    """The double sum of poly_overlap.h, evaluated in Fractions, is the slab checker's area: the rule itself is exact."""
    for name in ("triangle_L", "hole", "two_polygons", "coincident", "boxes_only", "rings_65/rev"):
        c = pc.case(name)
        for (t, d, g), e in pc.exact(name).items():
            inst = c["dets"][t][d]
            rings = [r for poly in inst for r in poly]
            roles = [1 if k == 0 else -1 for poly in inst for k in range(len(poly))]
            tp, tq = ref.edge_terms(ref.signed_edges(c["labels"][t][g], [1] * len(c["labels"][t][g])), ref.signed_edges(rings, roles))
            assert sum(tp) == e["A"] and sum(tq) == e["A"], (name, t, d, g)


# ---------------------------------------------------------------------------------------------------- the conditions on the cases
@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    """(a) every weight is decided: 100 A / area lies at least 1e-3 from any half-integer.  (b) po_bound <= 2^-20 px^2, and an edge
    that carries any part of the sum carries at least 1/16 px^2, so removing it or flipping its sign moves the exact area by far more
    than the bound.  (An edge with nothing of the other operand below it -- the lowest edges, the vertical ones -- carries exactly 0
    in the rule, whatever the shapes: for those 'any single edge' cannot hold, in any case; they are counted and printed.)"""
    c = pc.case(name)
    ex = pc.exact(name)
    carrying = idle = 0
    for (t, d, g), e in ex.items():
        q = e["A"] / e["area"] * 100
        half = q - q.__floor__() - Fraction(1, 2)
        assert abs(half) >= Fraction(1, 1000), (name, t, d, g, float(q))
        assert e["bound"] <= 2.0 ** -20, (name, t, d, g, e["bound"])
        if e["A"] == 0:
            continue
        inst = c["dets"][t][d]
        rings = [r for poly in inst for r in poly]
        roles = [1 if k == 0 else -1 for poly in inst for k in range(len(poly))]
        tp, tq = ref.edge_terms(ref.signed_edges(c["labels"][t][g], [1] * len(c["labels"][t][g])), ref.signed_edges(rings, roles))
        for v in tp + tq:
            if v == 0:
                idle += 1
            else:
                carrying += 1
                assert abs(v) >= Fraction(1, 16), (name, t, d, g, float(v))
    print(f"{name}: {len(ex)} pairs, {carrying} edges carry >= 1/16 px^2, {idle} carry nothing")


# ---------------------------------------------------------------------------------------------------- the host restatement
@pytest.mark.parametrize("name", NAMES)
def test_host_areas_within_po_bound(name):
    """|computed area - exact area| <= po_bound on every pair (raw_areas: the entry leaves the rounding out)."""
    c = pc.case(name)
    A, _, _ = rv.polygon_overlaps_host(pc.tables(c), gt_cap=pc.CAP, raw_areas=True)
    worst = 0.0
    for (t, d, g), e in pc.exact(name).items():
        err = abs(Fraction(float(A[t, d, g])) - e["A"])
        assert err <= Fraction(e["bound"]), (name, t, d, g, float(err), e["bound"])
        if not e["boxes_meet"]:
            assert A[t, d, g] == 0.0
        worst = max(worst, float(err) / e["bound"])
    print(f"{name}: worst error / po_bound = {worst:.3g}")


@pytest.mark.parametrize("name", NAMES)
def test_host_weights_are_the_rounding_of_the_exact_quotient(name):
    c = pc.case(name)
    frac, area, flagged = rv.polygon_overlaps_host(pc.tables(c), gt_cap=pc.CAP, prefill=7.0)
    ex = pc.exact(name)
    want = np.zeros_like(frac)
    for (t, d, g), e in ex.items():
        want[t, d, g] = pc.exact_frac(e["A"], e["area"])
        assert abs(area[t, g] - float(e["area"])) <= 2.0 ** -40, (name, t, g)
        if not e["boxes_meet"]:
            assert frac[t, d, g] == 0.0
    assert np.array_equal(frac, want), (name, np.argwhere(frac != want)[:5])
    assert flagged.tolist() == [sum(inst is None for inst in tile) for tile in c["dets"]]
    for t, tile in enumerate(c["labels"]):
        assert not area[t, len(tile):].any() and not frac[t, :, len(tile):].any()
        assert not frac[t, len(c["dets"][t]):].any()


def test_reversed_rings_give_the_same_weights():
    for c in pc.cases():
        if c["name"].endswith("/rev"):
            continue
        a = rv.polygon_overlaps_host(pc.tables(c), gt_cap=pc.CAP)
        b = rv.polygon_overlaps_host(pc.tables(pc.case(c["name"] + "/rev")), gt_cap=pc.CAP)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), c["name"]


def test_label_of_two_chunks():
    """A label of more than PO_STAGE edge slots is staged in two chunks; the area is the sum of both."""
    lab = pc.zigzag(pc.Q, 3 + pc.Q, 600, 7 + pc.Q, pc.Q / 4 * 0 + Fraction(1, 16))       # 598 top vertices over 37.3 px
    det = pc.comb(1, 2, 64, 5, 10)
    tabs = {**rv.stack_polygon_tables([pc.tile_tables([[[det]]])]),
            **rv.pack_label_pool([[[np.array([float(v) for q in lab for v in q])]]])}
    A, area, _ = rv.polygon_overlaps_host(tabs, gt_cap=1, raw_areas=True)
    want = ref.intersection_area([lab], [det])
    assert abs(Fraction(float(A[0, 0, 0])) - want) <= Fraction(pc.po_bound(600, 64, 40.0, 12.0))
    assert abs(Fraction(float(area[0, 0])) - ref.rings_area([lab])) <= Fraction(2.0 ** -40)


# ---------------------------------------------------------------------------------------------------- the sweep on the weights
def _sweep_batch(c):
    frac, _, _ = rv.polygon_overlaps_host(pc.tables(c), gt_cap=pc.CAP)
    t = pc.tables(c)
    return {"det_scores": c["det_scores"], "det_classes": c["det_classes"], "det_count": t["det_count"], "tile_first": t["tile_first"], "frac": frac}


@pytest.mark.parametrize("T", sorted(SWEEPS))
def test_area_sweep_slices_are_the_single_tables(T):
    for name in ("tiles", "rects", "two_polygons/rev"):
        b = _sweep_batch(pc.case(name))
        ws, wa, pr = rv.road_votes_area_sweep_host(b, 2, SWEEPS[T], prefill=5.0)
        assert ws.shape == (b["frac"].shape[0], T, pc.CAP, 2)
        for j, thr in enumerate(SWEEPS[T]):
            one = rv.road_votes_area_sweep_host(b, 2, [thr])
            for got, want in zip((ws, wa, pr), one):
                assert np.array_equal(got[:, j], want[:, 0]), (name, T, j)
        assert pr.sum() > 0


def test_area_sweep_is_the_rule_in_numpy():
    b = _sweep_batch(pc.case("tiles"))
    thr = 0.3
    ws, wa, pr = rv.road_votes_area_sweep_host(b, 2, [thr])
    n, D, cap = b["frac"].shape
    for t in range(n):
        G = int(b["tile_first"][t + 1] - b["tile_first"][t])
        for g in range(cap):
            for k in range(2):
                s_w = s_a = np.float64(0.0)
                cnt = 0
                for d in range(int(b["det_count"][t])):
                    f, sc = np.float64(b["frac"][t, d, g]), np.float64(b["det_scores"][t, d])
                    if g < G and int(b["det_classes"][t, d]) == k and f > 0.05 and sc >= thr:
                        s_w, s_a, cnt = s_w + f * sc, s_a + f, cnt + 1
                assert (ws[t, 0, g, k], wa[t, 0, g, k], pr[t, 0, g, k]) == (s_w, s_a, cnt)


def test_rectilinear_shapes_give_the_pixel_tables():
    """Unsimplified detections of rectilinear masks against integer-rectangle labels: every term is an integer or a half, float64 is
    exact, and the tables are those of rs_host_road_votes_sweep on the pixel counts, bit for bit."""
    from proj_roadsurf_amd.vectorize import vectorize_masks_native
    side, n_det = 32, 7
    rng = np.random.default_rng(5)
    masks = np.zeros((n_det, side, side), bool)
    for d in range(n_det):
        for _ in range(int(rng.integers(1, 4))):
            x0, y0 = rng.integers(0, side - 4, 2)
            x1, y1 = x0 + rng.integers(2, side - x0 + 1), y0 + rng.integers(2, side - y0 + 1)
            masks[d, y0:y1, x0:x1] = True
        if d % 2:
            masks[d, 10:14, 8:20] = False           # holes and split shapes
    packed = np.packbits(masks, axis=2, bitorder="little")
    labels = [[[np.array(pc.rect(*map(float, r)), np.float64).reshape(-1)] for r in ((2, 3, 30, 9), (5, 0, 9, 32), (0, 0, 32, 32), (20, 20, 21, 21), (11, 11, 17, 13))]]
    lab = rv.label_rasters(labels[0], side, side)
    inter = np.zeros((1, n_det, pc.CAP), np.int32)
    area = np.zeros((1, pc.CAP), np.int32)
    for g in range(len(labels[0])):
        inter[0, :, g] = rv._POP8[packed & lab[g][None]].sum(axis=(1, 2))
        area[0, g] = rv._POP8[lab[g]].sum()
    scores = rng.uniform(0.05, 1.0, (1, n_det)).astype(np.float32)
    classes = rng.integers(0, 2, (1, n_det)).astype(np.int32)
    first = np.array([0, len(labels[0])], np.int32)
    thr = SWEEPS[20]
    pixel = rv.road_votes_sweep_host({"det_scores": scores, "det_classes": classes, "det_count": np.array([n_det], np.int32), "tile_first": first,
                                      "inter": inter, "gt_area": area}, 2, thr)
    tabs = rv.polygon_tables_from_lists(vectorize_masks_native(packed, side, side, 0.0))
    b = {**rv.stack_polygon_tables([tabs]), **rv.pack_label_pool(labels)}
    frac, p_area, _ = rv.polygon_overlaps_host(b, gt_cap=pc.CAP)
    assert np.array_equal(p_area[0], area[0].astype(np.float64))
    poly = rv.road_votes_area_sweep_host({"det_scores": scores, "det_classes": classes, "det_count": b["det_count"], "tile_first": first, "frac": frac}, 2, thr)
    for got, want in zip(poly, pixel):
        assert np.array_equal(got, want)
    assert poly[2].sum() > 0
    # and the host route's tables are the same cells
    host = rv.vote_tables_polygons_host([tabs], labels, [scores[0]], [classes[0]], thr)[0]
    for got, want in zip(host[:3], pixel):
        assert np.array_equal(got, want[0, :, :len(labels[0])])


def test_host_route_takes_more_than_128_labels():
    c = pc.case("tiles")
    many = pc.float_labels(c)[2]
    labs = many + many[:5]
    tabs = pc.tile_tables(c["dets"][2])
    out = rv.vote_tables_polygons_host([tabs], [labs], [c["det_scores"][2, :2]], [c["det_classes"][2, :2]], [0.0])[0]
    assert out[0].shape == (1, 133, 2) and out[3].shape == (133,)
    assert np.array_equal(out[0][:, 128:], out[0][:, :5]) and np.array_equal(out[3][128:], out[3][:5])
    with pytest.raises(ValueError):
        rv.vote_tables_polygons_host([pc.tile_tables(c["dets"][3])], [[]], [c["det_scores"][3, :3]], [c["det_classes"][3, :3]], [0.0])   # a flagged instance


# ---------------------------------------------------------------------------------------------------- refusals
def _raw_overlaps(lib, b, n, slots, cap, null=None, device=False):
    dts = (np.int32, np.int32, np.int32, np.int16, np.int32, np.int32, np.int32, np.int32, np.int32, np.float64)
    tabs = [np.ascontiguousarray(b[k], dt) for k, dt in zip(rv.POLY_TABLE_KEYS, dts)]
    outs = [np.full((4096,), 7.0), np.full((512,), 7.0), np.full((8,), 7, np.int32)]
    ptrs = [a.ctypes.data for a in tabs + outs]
    if null is not None:
        ptrs[null] = None
    f = lib.rs_op_polygon_overlaps if device else lib.rs_host_polygon_overlaps
    f.argtypes = [C.c_void_p] * 10 + [C.c_int] * 4 + [C.c_void_p] * (4 if device else 3)
    rc = f(*ptrs[:10], n, slots, cap, 0, *ptrs[10:], *([None] if device else []))
    assert all((o == 7).all() for o in outs), "a refused call touched its outputs"
    return rc


def _raw_sweep(lib, entry, b, n, K, slots, cap, thr, T, area=False):
    tabs = [np.ascontiguousarray(b["det_scores"], np.float32), np.ascontiguousarray(b["det_classes"], np.int32), np.ascontiguousarray(b["det_count"], np.int32),
            np.ascontiguousarray(b["tile_first"], np.int32)]
    tabs += [np.ascontiguousarray(b["frac"], np.float64)] if area else [np.ascontiguousarray(b["inter"], np.int32), np.ascontiguousarray(b["gt_area"], np.int32)]
    outs = [np.full((4096,), 7.0), np.full((4096,), 7.0), np.full((4096,), 7, np.int32)]
    thr = np.ascontiguousarray(thr, np.float64)
    f = getattr(lib, entry)
    f.argtypes = [C.c_void_p] * len(tabs) + [C.c_int] * 4 + [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    rc = f(*[a.ctypes.data for a in tabs], n, K, slots, cap, thr.ctypes.data if thr.size else None, T, *[a.ctypes.data for a in outs])
    assert all((o == 7).all() for o in outs), "a refused call touched its outputs"
    return rc


def test_refusals_match_the_pixel_entries():
    lib = load_library()
    c = pc.case("rects")
    b = pc.tables(c)
    slots = b["header"].shape[1]
    sweep = dict(_sweep_batch(c), inter=np.zeros((1, slots, 4), np.int32), gt_area=np.zeros((1, 4), np.int32))
    sweep["frac"] = np.zeros((1, slots, 4))
    ok = [0.5]
    bad = [(0, 2, slots, 4, ok, 1), (1, 0, slots, 4, ok, 1), (1, 81, slots, 4, ok, 1), (1, 2, 0, 4, ok, 1), (1, 2, slots, 0, ok, 1),
           (1, 2, 1025, 4, ok, 1), (1, 2, slots, 129, ok, 1), (1, 2, slots, 4, ok, 0), (1, 2, slots, 4, ok * 33, 33),
           (1, 2, slots, 4, [np.nan], 1), (1, 2, slots, 4, [0.1, np.inf], 2), (1, 2, slots, 4, [], 1)]
    for n, K, D, cap, thr, T in bad:
        want = _raw_sweep(lib, "rs_host_road_votes_sweep", sweep, n, K, D, cap, thr, T)
        got = _raw_sweep(lib, "rs_host_road_votes_area_sweep", sweep, n, K, D, cap, thr, T, area=True)
        assert want != 0 and got == want, (n, K, D, cap, thr, T, got, want)
    # the overlaps: sizes as the vote's (the same codes), and every null table
    for n, D, cap in ((0, slots, 4), (1, 0, 4), (1, slots, 0), (1, 1025, 4), (1, slots, 129)):
        want = _raw_sweep(lib, "rs_host_road_votes_sweep", sweep, n, 2, D, cap, ok, 1)
        assert _raw_overlaps(lib, b, n, D, cap) == want != 0, (n, D, cap)
    arg = _raw_sweep(lib, "rs_host_road_votes_sweep", sweep, 0, 2, slots, 4, ok, 1)
    for k in range(13):
        assert _raw_overlaps(lib, b, 1, slots, 4, null=k) == arg, k
    with pytest.raises(RsError):
        rv.road_votes_area_sweep_host(sweep, 2, [np.nan])
    with pytest.raises(ValueError):
        rv.check_vote_geometry("polygons", vectorize="host")
    with pytest.raises(ValueError):
        rv.check_vote_geometry("voxels")
    assert rv.check_vote_geometry("pixels", vectorize="host") == "pixels"


def test_reduce_votes_takes_float64_areas():
    c = pc.case("tiles")
    t = pc.tables(c)
    host = rv.vote_tables_polygons_host([pc.tile_tables(tile) for tile in c["dets"][:3]], pc.float_labels(c)[:3],
                                        [c["det_scores"][i, :len(c["dets"][i])] for i in range(3)],
                                        [c["det_classes"][i, :len(c["dets"][i])] for i in range(3)], [0.0])
    assert all(h[3].dtype == np.float64 for h in host)
    ids = [[f"r{g % 40}" for g in range(len(tile))] for tile in c["labels"][:3]]
    rows = rv.reduce_votes([rv.sweep_slice(h, 0) for h in host], ids)
    as_int = rv.reduce_votes([rv.sweep_slice(h[:3] + (np.rint(h[3]).astype(np.int32),), 0) for h in host], ids)
    assert rows == as_int and len(rows) == 40
    assert {r["cover_type"] for r in rows} & {"artificial", "natural"}


def test_cli_refuses_the_geometry_up_front(tmp_path):
    """Before the configuration is read or a device touched: the file named here does not exist."""
    from proj_roadsurf_amd import make_detections
    cfg = str(tmp_path / "missing.yaml")
    for argv in ([cfg, "--road-votes", "--vote-geometry", "polygons"], [cfg, "--road-votes", "--vote-geometry", "polygons", "--vectorize", "host"],
                 [cfg, "--vectorize", "device", "--vote-geometry", "polygons"]):
        with pytest.raises(SystemExit) as e:
            make_detections.main(argv)
        assert "--vote-geometry polygons" in str(e.value)
    with pytest.raises(FileNotFoundError):                          # accepted: the run goes on to its configuration
        make_detections.main([cfg, "--road-votes", "--vectorize", "device", "--vote-geometry", "polygons"])
