#!/usr/bin/env python3
"""What the engine graph builder (csrc/engine.hip, over struct rs_engine of csrc/engine_internal.h; for a trainer, reached from csrc/trainer.hip) builds, one JSON record per configuration: structure (net shape, ordered stage
names, ordered tensor table), accounting and dispatch (flops / bytes / kernel per stage, conv variants) and output bits (sha256 of
every registered tensor's device buffer and of the returned detections).  Two manifests of the same machine are compared field for
field with ``--compare``: a change of the builder that is meant to keep behaviour must leave the manifest as it was.

    engine_manifest.py --out manifest.json [--fixture tests/golden/engine_structure.json] [--only NAME ...]
    engine_manifest.py --compare A.json B.json [--also-unstable-between C.json]

The structure part is host-side; tests/test_gpu_engine_structure.py holds it against tests/golden/engine_structure.json."""
import argparse
import ctypes as C
import hashlib
import json
import os
import re
import sys
from typing import Any, Dict, List, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from proj_roadsurf_amd.engine import Engine, RsError, Trainer, _check  # noqa: E402
from proj_roadsurf_amd.spec import EngineSpec  # noqa: E402
from proj_roadsurf_amd.synthetic import synthetic_tiles  # noqa: E402
from proj_roadsurf_amd.weights import synthetic_weights  # noqa: E402

BASE = dict(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300)
DEFAULT = "fp16"               # the configuration whose tensor table the fixture stores in full
DT_SIZE = {1: 2, 2: 4, 3: 4, 4: 1, 5: 2}
DT_SPLIT16 = 5

FP16_SWITCHES = ["RS_FUSE_STEM=0", "RS_FUSE_BNECK=0", "RS_FUSE_SHORTCUT=0", "RS_MERGE_LEVELS=0", "RS_FUSE_RPN_HEADS=0",
                 "RS_FUSE_MASK_PREDICTOR=0", "RS_CONV_DEEP=0", "RS_USE_GLDS=0", "RS_SIDE_STREAM=0", "RS_USE_GRAPH=1", "RS_ROI_ORDER=0",
                 "RS_NARROW_ROIALIGN=1"]
SPLIT_SWITCHES = ["RS_FUSE_STEM=0", "RS_FUSE_BNECK=0", "RS_FUSE_SHORTCUT=0", "RS_MERGE_LEVELS=0", "RS_FUSE_RPN_HEADS=0",
                  "RS_FUSE_MASK_PREDICTOR=0", "RS_CONV_DEEP=0", "RS_ROI_WINDOW=0"]


def configurations() -> List[Dict[str, Any]]:
    """name, kind ("engine" / "trainer"), precision, env, spec overrides, tile (h, w, c, seed)."""
    out: List[Dict[str, Any]] = []

    def add(name, precision, env=None, spec=None, tile=(256, 256, 3, 77), kind="engine"):
        out.append(dict(name=name, kind=kind, precision=precision, env=dict(env or {}), spec=dict(spec or {}), tile=tile))

    for p in ("fp16", "split", "fp32"):
        add(p, p)
    for sw in FP16_SWITCHES:
        add("fp16," + sw, "fp16", env=dict([sw.split("=")]))
    add("fp16,RS_FUSE_BNECK=0,RS_FUSE_SHORTCUT=0", "fp16", env={"RS_FUSE_BNECK": "0", "RS_FUSE_SHORTCUT": "0"})
    for sw in SPLIT_SWITCHES:
        add("split," + sw, "split", env=dict([sw.split("=")]))
    for p in ("fp16", "split"):
        add(p + ",mask_on=False", p, spec=dict(mask_on=False))
        add(p + ",num_classes=1", p, spec=dict(num_classes=1))
        add(p + ",num_classes=80", p, spec=dict(num_classes=80))
        add(p + ",batched_nms=torchvision", p, spec=dict(batched_nms="torchvision"))
        add(p + ",4band", p, spec=dict(pixel_mean=(103.53, 116.28, 123.675, 110.0), pixel_std=(1.0, 1.0, 1.0, 1.0)), tile=(256, 256, 4, 77))
        add(p + ",nonsquare", p, spec=dict(min_size_test=224, max_size_test=400, rpn_pre_nms_topk_test=200, rpn_post_nms_topk_test=200),
            tile=(200, 300, 3, 41))
    for p in ("fp16", "fp32"):
        add("trainer," + p, p, kind="trainer", tile=(256, 256, 3, 888))
    return out


def spec_of(cfg: Dict[str, Any]) -> EngineSpec:
    return EngineSpec(**dict(BASE, **cfg["spec"])).replace(precision=cfg["precision"])


class _Env:
    """The configuration's switches, set before the engine is created and cleared after it is closed."""

    def __init__(self, env: Dict[str, str]):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _tensor_raw(lib, fn, handle, name: str):
    p, dt, nd, halo = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
    dims = (C.c_int64 * 5)()
    _check(lib, fn(handle, name.encode(), C.byref(p), C.byref(dt), C.byref(nd), dims, C.byref(halo)), f"tensor {name}")
    return int(p.value or 0), dt.value, tuple(int(dims[i]) for i in range(nd.value)), halo.value


def tensor_table(lib, fn, handle, names: List[str]) -> List[str]:
    rows = []
    for n in names:
        _, dt, dims, halo = _tensor_raw(lib, fn, handle, n)
        rows.append(f"{n}|{dt}|{'x'.join(str(d) for d in dims)}|{halo}")
    return rows


def table_sha(rows: List[str]) -> str:
    return hashlib.sha256("\n".join(rows).encode()).hexdigest()


def tensor_hashes(lib, fn, handle, names: List[str], batch: int, max_batch: int) -> Dict[str, str]:
    """sha256 of the device buffer of every tensor, halo included; a tensor whose leading dimension is the engine's batch capacity is
    cut to the first ``batch`` images (both planes of a split tensor)."""
    out = {}
    for n in names:
        ptr, dt, dims, _ = _tensor_raw(lib, fn, handle, n)
        planes = 2 if dt == DT_SPLIT16 else 1
        plane_bytes = int(np.prod(dims, dtype=np.int64)) * DT_SIZE[dt]
        buf = np.empty(planes * plane_bytes, np.uint8)
        _check(lib, lib.rs_memcpy_d2h(buf.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), buf.nbytes), "rs_memcpy_d2h")
        if dims and dims[0] == max_batch and batch < max_batch:
            buf = np.ascontiguousarray(buf.reshape(planes, max_batch, -1)[:, :batch])
        out[n] = hashlib.sha256(buf.tobytes()).hexdigest()
    return out


def _sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def engine_structure(eng: Engine) -> Dict[str, Any]:
    names = eng.tensor_names()
    return {"net_shape": list(eng.net_shape()), "stages": [s["name"] for s in eng.stage_times()],
            "tensors": tensor_table(eng.lib, eng.lib.rs_engine_tensor, eng._h, names)}


def _trainer_targets():
    gb = [np.array([[20.0, 30.0, 120.0, 160.0]], np.float32), np.array([[100.0, 100.0, 260.0, 280.0], [10.0, 10.0, 60.0, 50.0]], np.float32)]
    gc = [np.array([0]), np.array([1, 1])]
    polys = [[[np.array([b[0], b[1], b[2], b[1], b[2], b[3], b[0], b[3]], np.float64)] for b in bs] for bs in gb]
    return gb, gc, polys


_W: Dict[str, Any] = {}


def _weights(cfg: Dict[str, Any]):
    key = repr(sorted(cfg["spec"].items()))                       # the synthetic weights do not depend on the precision
    if key not in _W:
        _W[key] = synthetic_weights(spec_of(cfg), seed=0)
    return _W[key]


def device_failed(message: str) -> bool:
    """True unless an RsError's code is one of the host-side refusals (argument, blob, unsupported): after a HIP error nothing more
    is started on the device."""
    m = re.search(r"failed \((-?\d+)\)", message)
    return m is None or int(m.group(1)) not in (-1, -3, -4)       # RS_ERR_ARG, RS_ERR_BLOB, RS_ERR_UNSUPPORTED (csrc/common.h)


def record(cfg: Dict[str, Any], structure_only: bool = False) -> Dict[str, Any]:
    """One configuration's record; a configuration that does not create is recorded with its error."""
    spec = spec_of(cfg)
    th, tw, tc, seed = cfg["tile"]
    W = _weights(cfg)
    rec: Dict[str, Any] = {"name": cfg["name"]}
    with _Env(cfg["env"]):
        try:
            if cfg["kind"] == "trainer":
                tr = Trainer(spec, W, (th, tw, tc), batch=2, loss_scale=64.0)
                eng = tr.inference_engine()
            else:
                tr = None
                eng = Engine(spec, W, (th, tw, tc), max_batch=4)
        except RsError as e:
            rec["error"] = str(e)
            return rec
        try:
            rec["structure"] = engine_structure(eng)
            if tr is not None:
                tnames = tr.tensor_names()
                rec["structure"]["trainer_tensors"] = tensor_table(tr.lib, tr.lib.rs_trainer_tensor, tr._h, tnames)
                tr.set_profiling(False)                            # host only: the trainer assembles its own stage list on this call
                rec["structure"]["trainer_stages"] = [s["name"] for s in tr.stage_times()]
            if structure_only:
                return rec
            if tr is not None:
                gb, gc, polys = _trainer_targets()
                tr.set_sampling(256, 0.5, 128, 0.25)
                losses = tr.train_step(synthetic_tiles(2, th, tw, tc, seed=seed), gb, gc, polys, seed=1)
                tr.sync()
                rec["losses"] = {k: float(v).hex() for k, v in losses.items()}
                rec["hashes"] = tensor_hashes(tr.lib, tr.lib.rs_trainer_tensor, tr._h, [n for n in tnames if n.startswith("g:")], 2, 2)
                rec["hashes"].update({"fwd:" + k: v for k, v in
                                      tensor_hashes(eng.lib, eng.lib.rs_engine_tensor, eng._h, eng.tensor_names(), 2, 2).items()})
                return rec
            tiles = synthetic_tiles(3, th, tw, tc, seed=seed)
            eng.set_profiling(1)
            eng.infer(tiles)
            rec["accounting"] = [{"name": s["name"], "flops": s["flops"], "bytes": s["bytes"], "kernel": s["kernel"]} for s in eng.stage_times()]
            eng.set_profiling(0)
            eng.infer(tiles)
            rec["variants_n3"] = eng.stage_variants()
            rec["hashes"] = tensor_hashes(eng.lib, eng.lib.rs_engine_tensor, eng._h, eng.tensor_names(), 3, 4)
            rec["infer_n1"] = []
            for _ in range(3):                                     # eager warm-up, graph capture, replay (where a graph is used)
                d = eng.infer(tiles[:1], want_probs=spec.mask_on)[0]
                rec["infer_n1"].append({"count": len(d), "boxes": _sha(d.pred_boxes), "scores": _sha(d.scores), "classes": _sha(d.pred_classes),
                                        "masks": _sha(d._packed), "mask_probs": _sha(d.mask_probs if spec.mask_on else None)})
            rec["variants_n1"] = eng.stage_variants()
        except RsError as e:                                       # created, but a forward fails: recorded like a failure to create
            rec["run_error"] = str(e)
        finally:
            eng.close()
            if tr is not None:
                tr.close()
    return rec


def fixture_of(manifest: Dict[str, Any]) -> Dict[str, Any]:
    """The structure part, compact: stage names and tensor count everywhere, the tensor table as a hash except for the default."""
    out = {}
    for name, rec in manifest.items():
        if "error" in rec:
            out[name] = {"error": rec["error"]}
            continue
        s = rec["structure"]
        f = {"net_shape": s["net_shape"], "stages": s["stages"], "tensor_count": len(s["tensors"])}
        if name == DEFAULT:
            f["tensors"] = s["tensors"]
        else:
            f["tensors_sha256"] = table_sha(s["tensors"])
        if "trainer_tensors" in s:
            f["trainer_stages"] = s["trainer_stages"]
            f["trainer_tensor_count"] = len(s["trainer_tensors"])
            f["trainer_tensors_sha256"] = table_sha(s["trainer_tensors"])
        out[name] = f
    return out


def fixture_text(fixture: Dict[str, Any]) -> str:
    """One configuration per line (the file stays small and a diff names the configuration)."""
    rows = [json.dumps(k) + ": " + json.dumps(fixture[k], sort_keys=True, separators=(",", ":")) for k in sorted(fixture)]
    return "{\n" + ",\n".join(rows) + "\n}\n"


def unstable_between(a: Dict[str, Any], b: Dict[str, Any]) -> List[str]:
    """"<configuration>/<tensor>" of every tensor hash that differs between two manifests of the same code."""
    out = []
    for name in a:
        ha, hb = a[name].get("hashes", {}), b.get(name, {}).get("hashes", {})
        out += [f"{name}/{t}" for t in ha if ha[t] != hb.get(t)]
    return out


def differences(a: Dict[str, Any], b: Dict[str, Any], skip: List[str]) -> List[str]:
    out = []
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name), b.get(name)
        if ra is None or rb is None:
            out.append(f"{name}: only in one manifest")
            continue
        for key in sorted(set(ra) | set(rb)):
            va, vb = ra.get(key), rb.get(key)
            if key == "hashes" and va is not None and vb is not None:
                for t in sorted(set(va) | set(vb)):
                    if va.get(t) != vb.get(t) and f"{name}/{t}" not in skip:
                        out.append(f"{name}: hash of {t} differs")
            elif va != vb:
                out.append(f"{name}: {key} differs")
    return out


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--fixture", help="also write the structure fixture (tests/golden/engine_structure.json)")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--also-unstable-between", metavar="C", help="with --compare A B: leave out the tensors whose hash differs between A and C")
    args = ap.parse_args(argv)
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        skip = unstable_between(a, json.load(open(args.also_unstable_between))) if args.also_unstable_between else []
        diff = differences(a, b, skip)
        print(json.dumps({"unstable": skip, "differences": diff}, indent=1))
        return 1 if diff else 0
    manifest = {}
    stopped = False
    for cfg in configurations():
        if args.only and cfg["name"] not in args.only:
            continue
        manifest[cfg["name"]] = record(cfg)
        print(cfg["name"], "->", manifest[cfg["name"]].get("error", "ok"), flush=True)
        rec = manifest[cfg["name"]]
        if "run_error" in rec or device_failed(rec.get("error", "failed (-1)")):   # the device failed: nothing more is started on it
            print("stopping:", rec.get("run_error", rec.get("error")), flush=True)
            stopped = True
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)
    if args.fixture:
        with open(args.fixture, "w") as f:
            f.write(fixture_text(fixture_of(manifest)))
    return 2 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
