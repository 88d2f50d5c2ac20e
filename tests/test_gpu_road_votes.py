"""The road cover vote on the device (csrc/road_vote.h, road_vote_kernel in csrc/val_ap.hip): the operator against the host
restatement bit for bit, ``Engine.road_votes`` against the numpy route on the masks the engine returns, behind every fetch form and
beside the validation counts that share its pool, the fallback of a batch that does not fit, and the streamed form of
``LanePipeline.run`` in both lane forms -- with and without labels."""
import numpy as np
import pytest

from proj_roadsurf_amd import raster_vote as RV
from proj_roadsurf_amd.engine import Engine, LanePipeline
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.synthetic import synthetic_tiles
from proj_roadsurf_amd.weights import synthetic_weights
from tests import road_vote_cases as V

pytestmark = pytest.mark.gpu
SPEC = dict(num_classes=2, min_size_test=192, max_size_test=320, rpn_pre_nms_topk_test=200, rpn_post_nms_topk_test=200)
THRESHOLD = 0.05


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("name", V.GPU_NAMES)
def test_operator_equals_host_restatement_bit_for_bit(gpu_required, name):
    b = V.case(name)
    want = RV.road_votes_host(b, b["num_classes"], b["threshold"])
    first = RV.road_votes_device(b, b["num_classes"], b["threshold"], prefill=-7.0)
    second = RV.road_votes_device(b, b["num_classes"], b["threshold"], prefill=3.0)    # whatever the buffers held: the operator clears them
    assert V.same_bits(first, want), [int((g != w).sum()) for g, w in zip(first, want)]
    assert V.same_bits(second, want)
    assert V.same_bits(want, V.expected(name)) and want[2].sum() > 0


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
    dets = eng.infer(tiles)
    labels = _labels_for(dets)
    want = RV.vote_tables_host(dets, labels, 2, THRESHOLD)           # the yardstick, once
    print(f"engine fixture: {[len(r) for r in dets]} detections, pairs per tile {[int(w[2].sum()) for w in want]}, label areas {[w[3].tolist() for w in want]}")
    assert sum(int(w[2].sum()) for w in want) > 0
    yield spec, W, tiles, eng, dets, labels, want
    eng.close()


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
            assert np.array_equal(g[0].pred_boxes.view(np.uint32), r.pred_boxes.view(np.uint32)) and not g[0].has("pred_masks")


def test_engine_votes_equal_the_numpy_route_on_its_masks(small):
    spec, W, tiles, eng, dets, labels, want = small
    _same(eng.road_votes(tiles, labels, THRESHOLD), want, dets)
    _same(eng.road_votes(tiles, labels, THRESHOLD), want, dets)       # the pool and the tables are reused
    assert eng.vote_fallbacks == 0 and eng.eval_fallbacks == 0
    one = eng.road_votes(tiles[:1], labels[:1], THRESHOLD)            # a ragged batch (and the one-tile path)
    ref1 = RV.vote_tables_host(eng.infer(tiles[:1]), labels[:1], 2, THRESHOLD)
    _same(one, ref1)
    other = eng.road_votes(tiles, labels, 0.5)                        # the threshold travels
    _same(other, RV.vote_tables_host(dets, labels, 2, 0.5))


@pytest.mark.parametrize("form", ["crops", "polygons", "canvas"])
def test_vote_follows_a_fetch_of_the_same_forward(small, form):
    spec, W, tiles, eng, dets, labels, want = small
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 2)
    eng.fetch_async(2, crops=form == "crops", polygons=form == "polygons")
    assert eng.road_votes(2, labels, THRESHOLD, wait=False) is True
    res = eng.fetch_wait(2)                                           # the fetch keeps its own wait
    got = eng.road_votes_wait(2)
    _same(got, want, dets)
    for r, d in zip(res, dets):
        assert np.array_equal(r.scores.view(np.uint32), d.scores.view(np.uint32))
        if form != "polygons":
            assert np.array_equal(r.pred_masks, d.pred_masks)
        else:
            assert r._polygons is not None
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 2)    # and the other order of the two waits
    eng.fetch_async(2, crops=form == "crops", polygons=form == "polygons")
    eng.road_votes(2, labels, THRESHOLD, wait=False)
    _same(eng.road_votes_wait(2), want, dets)
    res = eng.fetch_wait(2)
    if form != "polygons":
        assert all(np.array_equal(r.pred_masks, d.pred_masks) for r, d in zip(res, dets))


def test_validation_counts_share_the_pool_and_keep_their_results(small):
    spec, W, tiles, eng, dets, labels, want = small
    gts = [[[_rect(10.0, 10.0, 70.0, 50.0)], [_rect(64.0, 64.0, 128.0, 128.0)]], [[_rect(0.0, 0.0, 128.0, 128.0)]]]
    before = eng.eval_counts(tiles, gts)
    _same(eng.road_votes(tiles, labels, THRESHOLD), want, dets)
    after = eng.eval_counts(tiles, gts)
    for b, a in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(b[1:], a[1:]))
    assert after[1][3].tolist() == [128 * 128] and after[0][3].tolist() == [60 * 40, 64 * 64]
    _same(eng.road_votes(tiles, labels, THRESHOLD), want, dets)


def test_vote_taken_while_the_next_forward_runs(small):
    spec, W, tiles, eng, dets, labels, want = small
    assert eng.road_votes(tiles, labels, THRESHOLD, wait=False) is True
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles[::-1])), 2)
    _same(eng.road_votes_wait(2), want, dets)
    eng.sync()


# ------------------------------------------------------------------------------------------------ fallback and the streamed form
def _batches(tiles):
    return [tiles, tiles[::-1].copy(), tiles]


def test_a_tile_with_129_labels_does_not_fit(small):
    spec, W, tiles, eng, dets, labels, want = small
    many = [labels[0], [[_rect(10.0 + (i % 7), 10.0, 60.0, 70.0)] for i in range(129)]]
    assert eng.road_votes(tiles, many, THRESHOLD) is None and eng.vote_fallbacks == 1 and eng.eval_fallbacks == 0
    _same(eng.road_votes(tiles, labels, THRESHOLD), want, dets)       # the engine stays usable
    eng.vote_fallbacks = 0
    with pytest.raises(ValueError):
        eng.road_votes(tiles, labels[:1], THRESHOLD)
    with pytest.raises(ValueError):
        eng.road_votes(tiles, labels, float("nan"))


@pytest.fixture(scope="module", params=[False, True], ids=["independent_lanes", "shared_stream"])
def pipe(request, small):
    spec, W, tiles, eng, dets, labels, want = small
    p = LanePipeline(spec, W, (128, 128, 3), max_batch=2, lanes=2, shared_stream=request.param)
    yield p
    p.close()


def _bits(res):
    return [(r.pred_boxes.tobytes(), r.scores.tobytes(), r.pred_classes.tobytes(), r.pred_masks.tobytes()) for r in res]


def test_pipeline_with_labels_equals_the_single_engine(small, pipe):
    spec, W, tiles, eng, dets, labels, want = small
    batches = _batches(tiles)
    labs = [labels, labels[::-1], labels]
    wants = [[row[1:] for row in eng.road_votes(b, l, THRESHOLD)] for b, l in zip(batches, labs)]      # the single engine
    assert sum(int(row[2].sum()) for row in wants[1]) > 0
    plain = [_bits(res) for res in pipe.run(iter(batches))]
    names = [s["name"] for s in pipe.engines[0].stage_times()]
    assert len(names) > 10 and names == [s["name"] for s in eng.stage_times()]
    got = list(pipe.run(iter(batches), labels=iter(labs), vote_threshold=THRESHOLD))
    assert len(got) == 3 and pipe.vote_fallbacks == 0
    for res, w, p in zip(got, wants, plain):
        _same([r.road_votes for r in res], w)
        assert _bits(res) == p                                        # the detections are those of a run without labels
    # without labels again: the same bits, the same stages, no votes
    again = list(pipe.run(iter(batches)))
    assert [_bits(res) for res in again] == plain and all(not hasattr(r, "road_votes") for res in again for r in res)
    assert [s["name"] for s in pipe.engines[0].stage_times()] == names
    assert plain[0] == _bits(dets)


def test_pipeline_votes_an_oversized_batch_on_the_host(small, pipe):
    spec, W, tiles, eng, dets, labels, want = small
    many = [labels[0], [[_rect(10.0 + (i % 7), 10.0, 60.0, 70.0)] for i in range(129)]]
    labs = [labels, many, labels]
    got = list(pipe.run(iter(_batches(tiles)), labels=iter(labs), vote_threshold=THRESHOLD))
    assert pipe.vote_fallbacks == 1
    _same([r.road_votes for r in got[0]], want)
    _same([r.road_votes for r in got[2]], want)
    _same([r.road_votes for r in got[1]], RV.vote_tables_host(eng.infer(tiles[::-1].copy()), many, 2, THRESHOLD))
    assert got[1][1].road_votes[0].shape == (129, 2)


def test_pipeline_with_device_polygons_carries_votes(small):
    spec, W, tiles, eng, dets, labels, want = small
    p = LanePipeline(spec, W, (128, 128, 3), max_batch=2, lanes=2, vectorize="device")
    try:
        many = [labels[0], [[_rect(10.0 + (i % 7), 10.0, 60.0, 70.0)] for i in range(129)]]
        got = list(p.run(iter(_batches(tiles)), labels=iter([labels, many, labels]), vote_threshold=THRESHOLD))
        assert p.vote_fallbacks == 1 and all(r._polygons is not None for res in got for r in res)
        _same([r.road_votes for r in got[0]], want)
        _same([r.road_votes for r in got[1]], RV.vote_tables_host(eng.infer(tiles[::-1].copy()), many, 2, THRESHOLD))
        _same([r.road_votes for r in got[2]], want)
    finally:
        p.close()
