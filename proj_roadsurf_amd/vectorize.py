"""Detections -> vector features (host side).

What the object-detector's ``detectron2dets_to_features`` does after the predictor returns
([EXT od: helpers/detectron2.py], driven by R:config/config_obj_detec.yaml:87-89): each instance mask is
polygonised with ``rasterio.features.shapes`` (keep value 1), simplified with Ramer-Douglas-Peucker
(``rdp`` package, epsilon 0.75) and emitted as a feature ``{score, det_class, geometry}``.

rasterio, rdp and geopandas are not available offline; both algorithms are implemented in C++ in librs_engine.so
(csrc/vectorize.cpp, ``rs_vectorize_masks``): GDAL-polygonize semantics -- 4-connected regions of a binary mask, rings along
pixel edges (vertices only where the direction changes), exterior ring first, holes after it -- and the classic
Douglas-Peucker with perpendicular distance to the chord.  Multi-threaded over instances, straight on the bit-packed masks
the engine returns.  This module is the ctypes side only; the pure-Python restatement the C++ is checked against vertex for
vertex lives in oracle/host_tail_oracle.py (tests only).

PARITY UNPINNED against rasterio/rdp (absent); the unit tests pin areas, hole counts, documented conventions and invariants.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

Ring = List[Tuple[float, float]]
Polygon = List[Ring]                     # [exterior, hole, hole, ...], each ring closed (first == last)


def _effective_epsilon(rdp_enabled: bool, rdp_epsilon: float) -> float:
    return max(float(rdp_epsilon), 0.0) if rdp_enabled else 0.0


def _check_carried_epsilon(polygons, want: float) -> None:
    """Polygons that came with the instances were simplified on the device with ONE epsilon; asking for another one is an error,
    never a silent second vectorisation and never a silent acceptance."""
    if polygons.rdp_epsilon != want:
        raise ValueError(f"the instances carry polygons made with rdp epsilon {polygons.rdp_epsilon!r}, {want!r} was asked for "
                         "(0.0 = not simplified): fetch them with the epsilon you need, or fetch masks")


def _result_from_polygons(lib, polygons, crops, h: int, w: int, eps: float, threads: int):
    """``rs_vec_result*`` of one tile's instances from the tables the device polygoniser made (engine.PolygonTables); the flagged
    instances -- masks beyond the kernel's capacities -- are vectorised here from their crops and merged in slot order."""
    import ctypes as C
    from .engine import RsError
    hdr = polygons.header
    flagged = polygons.flagged
    fb = None
    if len(flagged):
        if crops is None:
            raise RsError(f"{len(flagged)} instance(s) were left to the host vectoriser but their masks did not come along")
        rects, offs, data = crops
        rects = np.ascontiguousarray(np.asarray(rects, np.int32)[flagged])
        offs = np.ascontiguousarray(np.asarray(offs, np.uint32)[flagged])
        data = np.ascontiguousarray(data, np.uint8)
        fb = lib.rs_vectorize_mask_crops(data.ctypes.data_as(C.c_void_p), rects.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                         len(flagged), h, w, float(eps), int(threads))
        if not fb:
            raise RsError("rs_vectorize_mask_crops failed")
    try:
        r = lib.rs_vec_from_tables(hdr.ctypes.data_as(C.c_void_p), hdr.shape[0], polygons.poly_ring_count.ctypes.data_as(C.c_void_p),
                                   polygons.ring_len.ctypes.data_as(C.c_void_p), polygons.xy.ctypes.data_as(C.c_void_p), fb)
    finally:
        if fb:
            lib.rs_vec_free(fb)
    if not r:
        raise RsError("rs_vec_from_tables: the polygon tables do not fit together")
    return r


def _nested_polygons(lib, r) -> List[List[Polygon]]:
    """The nested Python lists of an ``rs_vec_result*`` (not freed here)."""
    import ctypes as C
    c = [C.c_int64() for _ in range(4)]
    lib.rs_vec_counts(r, *[C.byref(x) for x in c])
    ni, npoly, nr, nv = (int(x.value) for x in c)
    ipc = np.zeros(ni, np.int32); prc = np.zeros(npoly, np.int32); rl = np.zeros(nr, np.int32); xy = np.zeros((nv, 2), np.float64)
    lib.rs_vec_copy(r, ipc.ctypes.data_as(C.POINTER(C.c_int32)), prc.ctypes.data_as(C.POINTER(C.c_int32)),
                    rl.ctypes.data_as(C.POINTER(C.c_int32)), xy.ctypes.data_as(C.POINTER(C.c_double)))
    out: List[List[Polygon]] = []
    pts = xy.tolist()
    pi = ri = vi = 0
    for i in range(ni):
        polys: List[Polygon] = []
        for _ in range(int(ipc[i])):
            rings: Polygon = []
            for _ in range(int(prc[pi])):
                k = int(rl[ri])
                rings.append([(p[0], p[1]) for p in pts[vi:vi + k]])
                vi += k
                ri += 1
            polys.append(rings)
            pi += 1
        out.append(polys)
    return out


def polygonize_masks_device(packed: np.ndarray, h: int, w: int, rdp_epsilon: float = 0.0, edge_cap: int = 0, vertex_cap: int = 0,
                            rects: Optional[np.ndarray] = None, det_count: Optional[np.ndarray] = None, slots: Optional[int] = None):
    """``rs_op_polygonize`` on n bit-packed masks (n, h, ceil(w/8)) uint8: uploads them, runs the device polygoniser
    (csrc/polygonize.hip) and returns ``engine.PolygonTables`` -- header flags included, nothing merged.  Caps of 0 = the
    kernel's defaults; smaller caps flag more instances (tests reach the fallback with small masks this way).
    ``rects`` (n, 4) int32 [first byte column, first row, bytes per row, rows], ``det_count`` (n / slots,) and ``slots``: the form
    the engine calls (``rs_op_polygonize_crops``) -- instance = tile * slots + slot, only the rectangle of a canvas is read, slots at
    or past their tile's count give all-zero headers."""
    import ctypes as C
    import torch
    from .engine import load_library, _check, PolygonTables, POLY_HDR
    lib = load_library()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n = packed.shape[0]
    if packed.shape[1:] != (h, (w + 7) // 8):
        raise ValueError(f"packed masks must be (n,{h},{(w + 7) // 8}), got {packed.shape}")
    if n == 0:
        return PolygonTables(np.zeros((0, POLY_HDR), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int16), rdp_epsilon)
    crop_form = rects is not None or det_count is not None or slots is not None
    slots = 1 if slots is None else int(slots)
    if slots < 1 or n % slots:
        raise ValueError(f"{n} masks are no whole number of tiles of {slots} slots")
    if rects is not None:
        rects = np.ascontiguousarray(rects, dtype=np.int32)
        if rects.shape != (n, 4):
            raise ValueError(f"rects must be ({n},4), got {rects.shape}")
    if det_count is not None:
        det_count = np.ascontiguousarray(det_count, dtype=np.int32)
        if det_count.shape != (n // slots,):
            raise ValueError(f"det_count must be ({n // slots},), got {det_count.shape}")
    caps = [C.c_int32() for _ in range(4)]
    lib.rs_polygonize_caps(*[C.byref(x) for x in caps])
    vcap, rcap = caps[1].value, caps[2].value
    dev = torch.device("cuda")
    m = torch.from_numpy(packed).to(dev)
    r_dev = torch.from_numpy(rects).to(dev) if rects is not None else None
    c_dev = torch.from_numpy(det_count).to(dev) if det_count is not None else None
    hdr = torch.zeros((n, POLY_HDR), dtype=torch.int32, device=dev)
    prc = torch.zeros(n * rcap, dtype=torch.int32, device=dev)
    rl = torch.zeros(n * rcap, dtype=torch.int32, device=dev)
    xy = torch.zeros((n * vcap, 2), dtype=torch.int16, device=dev)
    tot = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if crop_form:
        _check(lib, lib.rs_op_polygonize_crops(m.data_ptr(), n // slots, slots, c_dev.data_ptr() if c_dev is not None else None,
                                               r_dev.data_ptr() if r_dev is not None else None, h, w, float(rdp_epsilon), int(edge_cap), int(vertex_cap),
                                               hdr.data_ptr(), prc.data_ptr(), rl.data_ptr(), xy.data_ptr(), tot.data_ptr(), None), "rs_op_polygonize_crops")
    else:
        _check(lib, lib.rs_op_polygonize(m.data_ptr(), n, h, w, float(rdp_epsilon), int(edge_cap), int(vertex_cap), hdr.data_ptr(), prc.data_ptr(),
                                         rl.data_ptr(), xy.data_ptr(), tot.data_ptr(), None), "rs_op_polygonize")
    t = tot.cpu().numpy()
    return PolygonTables(hdr.cpu().numpy(), prc[:int(t[0])].cpu().numpy(), rl[:int(t[1])].cpu().numpy(), xy[:int(t[2])].cpu().numpy(), rdp_epsilon, totals=t)


def polygon_tables_to_lists(polygons, packed: Optional[np.ndarray], h: int, w: int, threads: int = 0) -> List[List[Polygon]]:
    """Nested polygon lists of ``PolygonTables`` (the form ``vectorize_masks_native`` returns); instances the device flagged are
    vectorised on the host from ``packed`` (their full canvases, (n, h, ceil(w/8))) with the tables' epsilon."""
    from .engine import load_library
    lib = load_library()
    crops = None
    if len(polygons.flagged):
        if packed is None:
            raise ValueError("flagged instances need their masks")
        packed = np.ascontiguousarray(packed, np.uint8)
        wb = (w + 7) // 8
        n = packed.shape[0]
        rects = np.tile(np.array([0, 0, wb, h], np.int32), (n, 1))
        offs = (np.arange(n, dtype=np.int64) * h * wb).astype(np.uint32)
        crops = (rects, offs, packed.reshape(-1))
    r = _result_from_polygons(lib, polygons, crops, h, w, polygons.rdp_epsilon, threads)
    try:
        return _nested_polygons(lib, r)
    finally:
        lib.rs_vec_free(r)


def vectorize_masks_native(packed: Optional[np.ndarray], h: int, w: int, rdp_epsilon: float = 0.0, threads: int = 0,
                           polygons=None, crops=None) -> List[List[Polygon]]:
    """Polygons of n bit-packed masks ``packed`` (n, h, ceil(w/8)) uint8 (LSB first, the engine's layout) through
    ``rs_vectorize_masks``: per instance a list of polygons, each a list of closed rings of (x, y) tuples --
    exactly ``[[rdp(r) ...] for poly in mask_to_polygons(mask)]`` of oracle/host_tail_oracle.py.  Raises if librs_engine.so is missing.
    ``polygons`` (engine.PolygonTables, as carried by ``Instances`` fetched with ``polygons=True``): the same lists from the tables
    the device made -- ``rdp_epsilon`` must be the one they carry (ValueError otherwise); ``crops``: the masks of flagged instances."""
    import ctypes as C
    from .engine import load_library, RsError
    lib = load_library()
    if polygons is not None:
        _check_carried_epsilon(polygons, max(float(rdp_epsilon), 0.0))
        if crops is None and packed is not None:
            return polygon_tables_to_lists(polygons, packed, h, w, threads)
        r = _result_from_polygons(lib, polygons, crops, h, w, polygons.rdp_epsilon, threads)
        try:
            return _nested_polygons(lib, r)
        finally:
            lib.rs_vec_free(r)
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n = packed.shape[0]
    if packed.shape[1:] != (h, (w + 7) // 8):
        raise ValueError(f"packed masks must be (n,{h},{(w + 7) // 8}), got {packed.shape}")
    if n == 0:
        return []
    r = lib.rs_vectorize_masks(packed.ctypes.data_as(C.c_void_p), n, h, w, float(rdp_epsilon), int(threads))
    if not r:
        raise RsError("rs_vectorize_masks failed")
    try:
        return _nested_polygons(lib, r)
    finally:
        lib.rs_vec_free(r)


def instances_to_gpkg_rows(instances, image_name: str, extent: Optional[Sequence[float]] = None, rdp_enabled: bool = True,
                           rdp_epsilon: float = 0.75, srs_id: int = -1, threads: int = 0):
    """The fast path of the CLI: masks -> polygons -> RDP -> georeferenced GeoPackage geometry blobs, all in C++
    (``rs_vectorize_masks`` + ``rs_vec_gpkg_blobs``); Python only pairs each blob with its instance's score and class.
    Returns (rows [(blob, score, det_class, image)], bbox [minx, miny, maxx, maxy] or None).  Same polygons, vertices and bytes as
    ``gpkg.gpkg_geom`` applied to ``instances_to_features`` (tests/test_vector_cli.py)."""
    import ctypes as C
    from .engine import load_library, RsError
    n = len(instances)
    carried = getattr(instances, "_polygons", None)
    if n == 0 or (carried is None and not instances.has("pred_masks")):
        return [], None
    lib = load_library()
    lib.rs_vec_gpkg_blobs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.rs_vec_gpkg_blobs.restype = C.c_int64
    h, w = instances.image_size
    crops = getattr(instances, "_crops", None)
    if carried is not None:
        # polygons arrived with the instances (made on the device): same rs_vec_result, same blobs
        eps_c = _effective_epsilon(rdp_enabled, rdp_epsilon)
        _check_carried_epsilon(carried, eps_c)
        r = _result_from_polygons(lib, carried, crops, h, w, eps_c, threads)
    elif crops is not None:
        # masks arrived as crops of their boxes (engine.Engine.fetch_wait, rs_mask_crops): trace inside the crops, same vertices
        rects, offs_c, data = crops
        lib.rs_vectorize_mask_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
        lib.rs_vectorize_mask_crops.restype = C.c_void_p
        rects = np.ascontiguousarray(rects, np.int32); offs_c = np.ascontiguousarray(offs_c, np.uint32); data = np.ascontiguousarray(data, np.uint8)
        r = lib.rs_vectorize_mask_crops(data.ctypes.data_as(C.c_void_p), rects.ctypes.data_as(C.c_void_p), offs_c.ctypes.data_as(C.c_void_p),
                                        n, h, w, float(rdp_epsilon if rdp_enabled else 0.0), int(threads))
    else:
        packed = getattr(instances, "_packed", None)
        if packed is None:
            packed = np.packbits(np.asarray(instances.pred_masks, dtype=bool), axis=2, bitorder="little")
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        r = lib.rs_vectorize_masks(packed.ctypes.data_as(C.c_void_p), n, h, w, float(rdp_epsilon if rdp_enabled else 0.0), int(threads))
    if not r:
        raise RsError("rs_vectorize_masks failed")
    try:
        c = [C.c_int64() for _ in range(4)]
        lib.rs_vec_counts(r, *[C.byref(x) for x in c])
        ni, npoly = int(c[0].value), int(c[1].value)
        if npoly == 0:
            return [], None
        ipc = np.zeros(ni, np.int32)
        lib.rs_vec_copy(r, ipc.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None)
        xform = None
        if extent is not None:
            xmin, ymin, xmax, ymax = (float(v) for v in extent)
            xform = np.ascontiguousarray(np.tile(np.array([xmin, ymax, (xmax - xmin) / w, (ymax - ymin) / h], np.float64), (ni, 1)))
        xp = xform.ctypes.data_as(C.c_void_p) if xform is not None else None
        need = int(lib.rs_vec_gpkg_blobs(r, xp, int(srs_id), None, 0, None, None))
        buf = np.empty(need, np.uint8)
        offs = np.zeros(npoly + 1, np.int64)
        bbox = np.zeros(4, np.float64)
        got = int(lib.rs_vec_gpkg_blobs(r, xp, int(srs_id), buf.ctypes.data_as(C.c_void_p), need, offs.ctypes.data_as(C.c_void_p), bbox.ctypes.data_as(C.c_void_p)))
        if got != need:
            raise RsError("rs_vec_gpkg_blobs failed")
    finally:
        lib.rs_vec_free(r)
    raw = buf.tobytes()
    o = offs.tolist()
    scores = [float(s) for s in instances.scores]
    classes = [int(k) for k in instances.pred_classes]
    inst_of = np.repeat(np.arange(ni), ipc).tolist()
    rows = [(raw[o[i]:o[i + 1]], scores[inst_of[i]], classes[inst_of[i]], image_name) for i in range(npoly)]
    return rows, bbox.tolist()


def instances_to_features(instances, image_name: str, extent: Optional[Sequence[float]] = None,
                          rdp_enabled: bool = True, rdp_epsilon: float = 0.75, threads: int = 0) -> List[dict]:
    """GeoJSON-like features, one per polygon, with the columns the reference's post-stage reads
    (``score``, ``det_class``, ``geometry`` -- R:scripts/road_segmentation/determine_class.py:22-25,113).
    ``extent`` = (xmin, ymin, xmax, ymax) of the tile in its CRS; None keeps pixel coordinates.
    The RDP tolerance is applied in pixel units, before georeferencing (documented assumption).
    Polygonisation and RDP run in C++ (``rs_vectorize_masks``); instances without masks give their boxes."""
    h, w = instances.image_size
    feats: List[dict] = []
    has_masks = instances.has("pred_masks")
    native_polys = None
    carried = getattr(instances, "_polygons", None)
    if carried is not None and len(instances):
        native_polys = vectorize_masks_native(None, h, w, _effective_epsilon(rdp_enabled, rdp_epsilon), threads, polygons=carried,
                                              crops=getattr(instances, "_crops", None))
    elif has_masks and len(instances):
        packed = getattr(instances, "_packed", None)
        if packed is None:          # a detectron2-style Instances with bool masks: pack them the way the engine does
            packed = np.packbits(np.asarray(instances.pred_masks, dtype=bool), axis=2, bitorder="little")
        native_polys = vectorize_masks_native(packed, h, w, rdp_epsilon if rdp_enabled else 0.0, threads)
    for i in range(len(instances)):
        if native_polys is None:
            x1, y1, x2, y2 = [float(v) for v in instances.pred_boxes[i]]
            polys: List[Polygon] = [[[(x1, y1), (x2, y1), (x2, y2), (x1, y2), (x1, y1)]]]
        else:
            polys = native_polys[i]
        for poly in polys:
            rings = []
            for r in poly:
                rr = list(r)
                if extent is not None:
                    xmin, ymin, xmax, ymax = extent
                    sx, sy = (xmax - xmin) / w, (ymax - ymin) / h
                    rr = [(xmin + x * sx, ymax - y * sy) for x, y in rr]
                rings.append([[float(x), float(y)] for x, y in rr])
            feats.append({"type": "Feature",
                          "geometry": {"type": "Polygon", "coordinates": rings},
                          "properties": {"score": float(instances.scores[i]), "det_class": int(instances.pred_classes[i]),
                                         "image": image_name}})
    return feats
