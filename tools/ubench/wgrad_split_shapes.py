#!/usr/bin/env python3
"""rs_op_conv2d_wgrad_f32 against rs_op_conv2d_wgrad_split per training-relevant layer shape (batch 8, 800x800 network input).

    python tools/ubench/wgrad_split_shapes.py [--rounds 7] [--reps 3] [--out DIR]

The two operators run interleaved -- f32, split, f32, ... -- each timed window being `reps` calls closed by a device synchronise; the
median and the spread (min, max) of the windows are reported.  The split figure includes the abs-max and the plane pass.  Both
operators allocate their scratch per call (two hipMalloc / hipFree pairs and a memset; the split operator's allocation also holds the
planes), so the kernels themselves are a little faster than printed, on both sides.  TFLOP/s count the layer's 2 M K Cout, not the three
fp16 products.  Prints one JSON line and writes it to DIR/wgrad_split_shapes.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N = 8
SHAPES = [  # name, cin, cout, k, stride, h, w
    ("fpn_output2 / rpn.conv p2 (3x3 256->256)", 256, 256, 3, 1, 200, 200),
    ("res4.x.conv1 (1x1 1024->256)", 1024, 256, 1, 1, 50, 50),
    ("res4.x.conv3 (1x1 256->1024)", 256, 1024, 1, 1, 50, 50),
    ("rpn.heads p2 (1x1 256->16)", 256, 16, 1, 1, 200, 200),
    ("box.fc1 (8192 x 12544 -> 1024)", 12544, 1024, 1, 1, 8192, 1),
]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wgrad_split_shapes.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.engine import load_library, _check
    lib = load_library()
    dev = torch.device("cuda:0")
    out = {"tool": "tools/ubench/wgrad_split_shapes.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps_per_window": args.reps,
           "shapes": []}
    for name, cin, cout, k, stride, h, w in SHAPES:
        pad = k // 2
        halo = 1 if k == 3 else 0
        n = N if w > 1 else 1
        x = torch.randn(n, h + 2 * halo, w + 2 * halo, cin, device=dev)
        dy = torch.randn(n, h + 2 * halo, w + 2 * halo, cout, device=dev) * 1e-3
        if halo:
            for t in (x, dy):
                t[:, 0] = 0; t[:, -1] = 0; t[:, :, 0] = 0; t[:, :, -1] = 0
        kpad = k * k * cin
        g = {m: torch.empty(cout, kpad, device=dev) for m in ("f32", "split")}

        def window(mode, reps):
            fn = lib.rs_op_conv2d_wgrad_f32 if mode == "f32" else lib.rs_op_conv2d_wgrad_split
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                _check(lib, fn(C.c_void_p(dy.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(g[mode].data_ptr()), None,
                               n, h, w, cin, halo, k, k, stride, pad, cout, kpad, halo, 0, None), name)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3
        for m in g:
            window(m, 2)
        ms = {m: [] for m in g}
        for r in range(args.rounds):
            for m in (("f32", "split") if r % 2 == 0 else ("split", "f32")):
                ms[m].append(window(m, args.reps))
        fl = 2.0 * n * h * w * k * k * cin * cout
        ref = g["f32"].double()
        rec = {"shape": name, "gflop": fl / 1e9, "served_by_the_split_kernel": bool(lib.rs_op_conv2d_wgrad_split_serves(cin, cout)),
               "rel_l2_split_vs_f32": float((g["split"].double() - ref).norm() / ref.norm())}
        for m in g:
            med = statistics.median(ms[m])
            rec[m] = {"ms_windows": [round(v, 4) for v in ms[m]], "ms_median": med, "ms_min": min(ms[m]), "ms_max": max(ms[m]), "tflops_median": fl / med / 1e9}
        rec["speedup_median"] = rec["f32"]["ms_median"] / rec["split"]["ms_median"]
        out["shapes"].append(rec)
        print(f"{name:42s} f32 {rec['f32']['ms_median']:8.3f} ms {rec['f32']['tflops_median']:6.1f} TFLOP/s   split {rec['split']['ms_median']:8.3f} ms "
              f"{rec['split']['tflops_median']:6.1f} TFLOP/s   x{rec['speedup_median']:.2f}   rel L2 {rec['rel_l2_split_vs_f32']:.1e}", file=sys.stderr, flush=True)
        del x, dy, g
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "wgrad_split_shapes.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
