"""The vote sweep on the device (csrc/road_vote.h THE SWEEP, road_vote_sweep_kernel in csrc/val_ap.hip): the operator against the host
restatement bit for bit at 1, 20 and 32 thresholds, ``Engine.road_votes_sweep`` against the numpy route on the masks the engine
returns and against ``Engine.road_votes`` on the same forward, behind every fetch form, the fallback of a batch that does not fit,
and the streamed form of ``LanePipeline.run``."""
import numpy as np
import pytest

from proj_roadsurf_amd import raster_vote as RV
from proj_roadsurf_amd.engine import Engine, LanePipeline
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.synthetic import synthetic_tiles
from proj_roadsurf_amd.weights import synthetic_weights
from tests import road_vote_cases as V
from tests import vote_sweep_cases as S

pytestmark = pytest.mark.gpu
SPEC = dict(num_classes=2, min_size_test=192, max_size_test=320, rpn_pre_nms_topk_test=200, rpn_post_nms_topk_test=200)
THRESHOLDS = np.array([0.05, 0.5, 0.0, 0.5, 0.3], np.float64)          # unsorted, a duplicate; the last is the vote's own below
SWEEP_NAMES = S.SLICE_NAMES + ("slots100", "random4")


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("which", sorted(S.LISTS))
@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_operator_equals_host_restatement_bit_for_bit(gpu_required, name, which):
    b, thr = V.case(name), S.LISTS[which]
    K = b["num_classes"]
    want = RV.road_votes_sweep_host(b, K, thr)
    first = RV.road_votes_sweep_device(b, K, thr, prefill=-7.0)
    second = RV.road_votes_sweep_device(b, K, thr, prefill=3.0)       # whatever the buffers held: the operator clears them
    assert V.same_bits(first, want), [int((g != w).sum()) for g, w in zip(first, want)]
    assert V.same_bits(second, want)
    assert first[0].shape == (len(b["det_count"]), thr.size, V.CAP, K) and want[2].sum() > 0
    j = thr.size // 2                                                  # and a slice against the single-threshold kernel
    assert V.same_bits(S.slice_of(first, j), RV.road_votes_device(b, K, float(thr[j])))


def test_operator_on_the_mixed_list_and_the_float32_boundaries(gpu_required):
    for name in S.SLICE_NAMES:
        b = V.case(name)
        assert V.same_bits(RV.road_votes_sweep_device(b, b["num_classes"], S.MIXED, prefill=1.0), RV.road_votes_sweep_host(b, b["num_classes"], S.MIXED)), name
    b = S.boundary_case()
    got = RV.road_votes_sweep_device(b, 1, S.REFERENCE)
    assert V.same_bits(got, RV.road_votes_sweep_host(b, 1, S.REFERENCE))
    sides = [bool(np.float64(np.float32(t)) >= np.float64(t)) for t in S.REFERENCE]
    assert got[2][0, :, 0, 0].tolist() == [19 - j + int(s) for j, s in enumerate(sides)]


# ------------------------------------------------------------------------------------------------ engine
def _rect(x0, y0, x1, y1):
    return np.array([x0, y0, x1, y0, x1, y1, x0, y1], np.float64)


def _labels_for(dets):
    """Three labels per tile: the bounding rectangle of the tile's largest mask (so that pairs exist), a band across the tile, and a
    label of two rings."""
    out = []
    for r in dets:
        m = r.pred_masks if len(r) else np.zeros((0, 128, 128), bool)
        big = int(m.reshape(len(r), -1).sum(1).argmax()) if len(r) and m.any() else -1
        if big >= 0:
            ys, xs = np.nonzero(m[big])
            own = _rect(float(xs.min()), float(ys.min()), float(xs.max() + 1), float(ys.max() + 1))
        else:
            own = _rect(30.0, 30.0, 90.0, 90.0)
        out.append([[own], [_rect(0.0, 40.5, 128.0, 80.25)], [_rect(5.0, 5.0, 40.0, 60.0), _rect(70.5, 64.0, 120.0, 127.0)]])
    return out


@pytest.fixture(scope="module")
def small(gpu_required):
    spec = EngineSpec(**SPEC)
    W = synthetic_weights(spec, 0)
    tiles = synthetic_tiles(2, 128, 128, 3, seed=5)
    eng = Engine(spec, W, (128, 128, 3), max_batch=2)
    names, tensors = [s["name"] for s in eng.stage_times()], _tensor_table(eng)       # before the first sweep
    dets = eng.infer(tiles)
    labels = _labels_for(dets)
    want = RV.vote_tables_host(dets, labels, 2, thresholds=THRESHOLDS)      # the yardstick, once
    print(f"engine fixture: {[len(r) for r in dets]} detections, pairs per tile and threshold {[w[2].sum(axis=(1, 2)).tolist() for w in want]}")
    assert sum(int(w[2].sum()) for w in want) > 0
    yield spec, W, tiles, eng, dets, labels, want, names, tensors
    eng.close()


def _tensor_table(eng):
    return eng.tensor_names()


def _same(got, want, dets=None):
    assert got is not None and len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g = g[-4:]
        assert [a.shape for a in g] == [a.shape for a in w] and g[0].dtype == np.float64 and g[2].dtype == np.int32
        for k in range(4):
            assert np.array_equal(g[k], w[k]), (i, k)
        assert V.same_bits(g[:2], w[:2])
    if dets is not None:
        for g, r in zip(got, dets):
            assert np.array_equal(g[0].scores.view(np.uint32), r.scores.view(np.uint32)) and np.array_equal(g[0].pred_classes, r.pred_classes)
            assert not g[0].has("pred_masks")


def test_engine_sweep_equals_the_numpy_route_and_the_single_vote(small):
    spec, W, tiles, eng, dets, labels, want, names, tensors = small
    got = eng.road_votes_sweep(tiles, labels, THRESHOLDS)
    _same(got, want, dets)
    assert got[0][1].shape == (THRESHOLDS.size, 3, 2)
    _same(eng.road_votes_sweep(tiles, labels, THRESHOLDS), want, dets)          # the pool and the tables are reused
    assert eng.vote_fallbacks == 0 and eng.eval_fallbacks == 0
    # the last slice against Engine.road_votes at that threshold, on the same forward
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 2)
    assert eng.road_votes_sweep(2, labels, THRESHOLDS, wait=False) is True
    sweep = eng.road_votes_sweep_wait(2)
    single = eng.road_votes(2, labels, float(THRESHOLDS[-1]))
    _same([RV.sweep_slice(row[1:], THRESHOLDS.size - 1) for row in sweep], [row[1:] for row in single])
    _same(single, RV.vote_tables_host(dets, labels, 2, float(THRESHOLDS[-1])))
    # one threshold, 32 thresholds, a ragged batch
    _same(eng.road_votes_sweep(tiles, labels, [0.3]), RV.vote_tables_host(dets, labels, 2, thresholds=[0.3]), dets)
    _same(eng.road_votes_sweep(tiles, labels, S.FULL), RV.vote_tables_host(dets, labels, 2, thresholds=S.FULL), dets)
    one = eng.road_votes_sweep(tiles[:1], labels[:1], THRESHOLDS)
    _same(one, RV.vote_tables_host(eng.infer(tiles[:1]), labels[:1], 2, thresholds=THRESHOLDS))
    # the sweep added no stage and no tensor
    assert [s["name"] for s in eng.stage_times()] == names and _tensor_table(eng) == tensors and len(names) > 10


@pytest.mark.parametrize("form", ["crops", "polygons", "canvas"])
def test_sweep_follows_a_fetch_of_the_same_forward(small, form):
    spec, W, tiles, eng, dets, labels, want, names, tensors = small
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 2)
    eng.fetch_async(2, crops=form == "crops", polygons=form == "polygons")
    assert eng.road_votes_sweep(2, labels, THRESHOLDS, wait=False) is True
    res = eng.fetch_wait(2)                                           # the fetch keeps its own wait
    _same(eng.road_votes_sweep_wait(2), want, dets)
    for r, d in zip(res, dets):
        assert np.array_equal(r.scores.view(np.uint32), d.scores.view(np.uint32))
        if form != "polygons":
            assert np.array_equal(r.pred_masks, d.pred_masks)
        else:
            assert r._polygons is not None


def test_a_tile_with_129_labels_does_not_fit(small):
    spec, W, tiles, eng, dets, labels, want, names, tensors = small
    many = [labels[0], [[_rect(10.0 + (i % 7), 10.0, 60.0, 70.0)] for i in range(129)]]
    before = eng.vote_fallbacks
    assert eng.road_votes_sweep(tiles, many, THRESHOLDS) is None and eng.vote_fallbacks == before + 1 and eng.eval_fallbacks == 0
    _same(eng.road_votes_sweep(tiles, labels, THRESHOLDS), want, dets)          # the engine stays usable
    eng.vote_fallbacks = 0
    for bad in ([], [0.1] * 33, [0.1, float("inf")]):
        with pytest.raises(ValueError):
            eng.road_votes_sweep(tiles, labels, bad)


def test_an_engine_that_never_sweeps_has_the_same_stages_and_tensors(small):
    spec, W, tiles, eng, dets, labels, want, names, tensors = small
    other = Engine(spec, W, (128, 128, 3), max_batch=2)
    try:
        other.infer(tiles)
        assert [s["name"] for s in other.stage_times()] == names and _tensor_table(other) == tensors
        assert other._sweep_struct is None
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------ the streamed form
def _batches(tiles):
    return [tiles, tiles[::-1].copy(), tiles]


@pytest.fixture(scope="module", params=[False, True], ids=["independent_lanes", "shared_stream"])
def pipe(request, small):
    spec, W, tiles = small[:3]
    p = LanePipeline(spec, W, (128, 128, 3), max_batch=2, lanes=2, shared_stream=request.param)
    yield p
    p.close()


def test_pipeline_sweep_with_votes_gives_the_votes_of_a_run_without(small, pipe):
    spec, W, tiles, eng, dets, labels, want, names, tensors = small
    batches, labs = _batches(tiles), [labels, labels[::-1], labels]
    user, thr = THRESHOLDS[:-1], float(THRESHOLDS[-1])
    alone = list(pipe.run(iter(batches), labels=iter(labs), vote_threshold=thr))
    both = list(pipe.run(iter(batches), labels=iter(labs), vote_threshold=thr, vote_sweep=user))
    assert len(both) == 3 and pipe.vote_fallbacks == 0
    for res_a, res_b in zip(alone, both):
        _same([r.road_votes for r in res_b], [r.road_votes for r in res_a])
        assert all(r.road_vote_sweep[0].shape[0] == user.size for r in res_b)
        assert [r.scores.tobytes() for r in res_a] == [r.scores.tobytes() for r in res_b]
    _same([r.road_vote_sweep for r in both[0]], [(w[0][:-1], w[1][:-1], w[2][:-1], w[3]) for w in want])
    _same([r.road_votes for r in both[0]], [RV.sweep_slice(w, THRESHOLDS.size - 1) for w in want])
    only = list(pipe.run(iter(batches), labels=iter(labs), road_votes=False, vote_sweep=THRESHOLDS))       # the sweep alone
    _same([r.road_vote_sweep for r in only[2]], want)
    assert all(not hasattr(r, "road_votes") for res in only for r in res)
    with pytest.raises(ValueError):
        list(pipe.run(iter(batches), vote_sweep=THRESHOLDS))                                              # needs labels


def test_pipeline_sweeps_an_oversized_batch_on_the_host(small, pipe):
    spec, W, tiles, eng, dets, labels, want, names, tensors = small
    many = [labels[0], [[_rect(10.0 + (i % 7), 10.0, 60.0, 70.0)] for i in range(129)]]
    user, thr = THRESHOLDS[:-1], float(THRESHOLDS[-1])
    got = list(pipe.run(iter(_batches(tiles)), labels=iter([labels, many, labels]), vote_threshold=thr, vote_sweep=user))
    assert pipe.vote_fallbacks == 1
    cut = lambda rows: [(w[0][:-1], w[1][:-1], w[2][:-1], w[3]) for w in rows]
    _same([r.road_vote_sweep for r in got[0]], cut(want))
    _same([r.road_vote_sweep for r in got[2]], cut(want))
    host = RV.vote_tables_host(eng.infer(tiles[::-1].copy()), many, 2, thresholds=THRESHOLDS)
    _same([r.road_vote_sweep for r in got[1]], cut(host))
    _same([r.road_votes for r in got[1]], [RV.sweep_slice(w, THRESHOLDS.size - 1) for w in host])
    assert got[1][1].road_vote_sweep[0].shape == (user.size, 129, 2)
