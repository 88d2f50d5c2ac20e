"""Cost of the box tail by class count: Engine.stage_times() of box.candidates, box.nms and box.merge_postprocess for 2, 8 and 80 classes
(8 is the last count of the one-launch forms, 80 takes the many-class forms: DESIGN.md 3.3) at batch 1 and batch 16, in one process, beside
the sum over all stages and the wall time of an unprofiled forward.  usage: many_classes.py [precision] [reps] [score_thresh_test]"""
import sys
import time

sys.path.insert(0, ".")
from proj_roadsurf_amd.engine import Engine                # noqa: E402
from proj_roadsurf_amd.spec import EngineSpec              # noqa: E402
from proj_roadsurf_amd.synthetic import synthetic_tiles    # noqa: E402
from proj_roadsurf_amd.weights import synthetic_weights    # noqa: E402

TAIL = ("box.candidates", "box.nms", "box.merge_postprocess")


def main():
    prec = sys.argv[1] if len(sys.argv) > 1 else "split"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    thr = float(sys.argv[3]) if len(sys.argv) > 3 else EngineSpec().score_thresh_test
    tiles = synthetic_tiles(16, 512, 512, 3, seed=3)
    print(f"precision {prec}, {reps} forwards per row, SCORE_THRESH_TEST {thr}; times in ms per forward", flush=True)
    print(f"{'K':>3} {'batch':>5} " + " ".join(f"{n:>22}" for n in TAIL) + f" {'all stages':>11} {'wall':>8}  candidates/img (classes)  detections/img", flush=True)
    for K in (2, 8, 80):
        spec = EngineSpec(num_classes=K, precision=prec, score_thresh_test=thr)
        W = synthetic_weights(spec, seed=0)
        for nb in (1, 16):
            e = Engine(spec, W, (512, 512, 3), max_batch=nb)
            try:
                ptr = e.upload_tiles(tiles[:nb])
                for _ in range(5):
                    e.infer_device(ptr, nb)
                    e.sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    e.infer_device(ptr, nb)
                    e.sync()
                wall = (time.perf_counter() - t0) / reps * 1e3
                e.set_profiling(2)
                before = {s["name"]: (s["ms_total"], s["calls"]) for s in e.stage_times()}
                for _ in range(reps):
                    e.infer_device(ptr, nb)
                    e.sync()
                ms = {}
                for s in e.stage_times():
                    calls = s["calls"] - before[s["name"]][1]
                    ms[s["name"]] = (s["ms_total"] - before[s["name"]][0]) / max(calls, 1)
                e.set_profiling(0)
                sc = e.tensor("box_seg_count", n=nb)
                dc = e.tensor("det_count", n=nb)
                print(f"{K:>3} {nb:>5} " + " ".join(f"{ms[n]:>22.4f}" for n in TAIL) + f" {sum(ms.values()):>11.3f} {wall:>8.3f}  "
                      f"{sc.sum(axis=1).mean():.0f} ({(sc > 0).sum(axis=1).mean():.1f})  {dc.mean():.1f}", flush=True)
            finally:
                e.close()


if __name__ == "__main__":
    main()
