"""GPU: two video streams' frames through ONE conv stack per launch (vnect_set_stream_batch / vnect_submit_streams, ABI v7).

The reference runs one estimator per video (run_estimator_ps.py:120-129); every stream served by a batched handle must get, frame by frame,
exactly the joints a handle of its own returns for that video."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0 = 1.7e9
PRECISIONS = {"fp32": 0, "bf16": 1, "fp32_split": 2}


def _make(weights, scales, **kw):
    from vnect_amd import _native
    h = _native.Handle(scales, num_frame_slots=8, **kw)
    h.set_weights(weights)
    h.finalize()
    return h


def _videos(n):
    """Two videos of different sizes -- the second fed as a strided crop of a larger frame -- and a third one.  The second alternates
    between a (260, 368) crop, whose squarify step is a copy (the batch's stem then builds both frames' pyramids itself), and a (240, 320)
    crop, which must be resized (pyramid_streams_kernel + the stem from the batch tensor)."""
    from tests import helpers
    a = [helpers.synth_frame(9100 + k, 368, 368, smooth=True) for k in range(n)]
    b = [helpers.synth_frame(9200 + k, 300, 420, smooth=True)[13:273, 31:399] if k % 2 == 0 else
         helpers.synth_frame(9200 + k, 300, 420, smooth=True)[13:253, 31:351] for k in range(n)]   # strided views, row stride 1 260
    c = [helpers.synth_frame(9300 + k, 368, 200, smooth=True) for k in range(n)]
    return [a, b, c]


def _times(n):
    return [[T0 + 7 * s + 0.033 * k + 0.004 * ((k * (s + 3)) % 5) for k in range(n)] for s in range(3)]


def _own(weights, scales, prec, vids, times):
    out = []
    for s in range(len(vids)):
        h = _make(weights, scales, precision=prec)
        out.append([h.infer(vids[s][k], times[s][k], times[s][k] + 0.0005) for k in range(len(vids[s]))])
        h.close()
    return out


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
@pytest.mark.parametrize("scales", [[1.0, 0.8, 0.6], [1.0, 0.7], [1.0], [1.0, 0.9, 0.75, 0.6]], ids=["s3", "s2", "s1", "s4"])
def test_batched_streams_equal_handles_of_their_own(weights, prec, scales):
    """Streams 0 and 1 as batches of two (8 batches, irregular timestamps), stream 2 submitted singly in between on the same handle.
    Four scales: 8 images per launch, the largest batch the ABI admits (2 S <= VNECT_MAX_SCALES)."""
    n = 8
    vids, times = _videos(n), _times(n)
    want = _own(weights, scales, PRECISIONS[prec], vids, times)
    h = _make(weights, scales, precision=PRECISIONS[prec], stream_batch=2)
    got, kc = [[], [], []], 0
    for k in range(n):
        h.upload_frame(0, vids[0][k])
        h.upload_frame(1, vids[1][k])
        h.submit_streams([0, 1], [0, 1], [times[0][k], times[1][k]], [times[0][k] + 0.0005, times[1][k] + 0.0005])
        for s in (0, 1):
            rs, j2, j3 = h.collect_stream()
            assert rs == s
            got[s].append((j2, j3))
        if k % 3 != 1:   # the third video: single submits between the batches, irregularly
            h.upload_frame(2, vids[2][kc])
            h.submit_stream(2, 2, times[2][kc], times[2][kc] + 0.0005)
            rs, j2, j3 = h.collect_stream()
            assert rs == 2
            got[2].append((j2, j3))
            kc += 1
    for s in range(3):
        for k in range(len(got[s])):
            assert _same(got[s][k], want[s][k]), (prec, scales, s, k)


def _forward_of_two_batches(weights, prec, scales):
    from tests import helpers
    S = len(scales)
    h = _make(weights, scales, precision=PRECISIONS[prec], stream_batch=2)
    x = np.stack([helpers.synth_frame(9400 + i, smooth=True).astype(np.float32) / 255.0 - 0.4 for i in range(2 * S)])
    one = np.concatenate([h.forward(x[:S]), h.forward(x[S:])])
    both = h.forward(x)
    assert both.shape == (2 * S, 46, 46, 84) and np.array_equal(both, one)
    swapped = h.forward(np.concatenate([x[S:], x[:S]]))
    assert np.array_equal(swapped, np.concatenate([one[S:], one[:S]]))


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_forward_of_two_batches_equals_two_forwards(weights, prec):
    _forward_of_two_batches(weights, prec, [1.0, 0.8, 0.6])


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_forward_of_two_four_scale_batches_equals_two_forwards(weights, prec):
    """8 images per launch: the largest batch the ABI admits"""
    _forward_of_two_batches(weights, prec, [1.0, 0.9, 0.75, 0.6])


def test_two_streams_of_five_scales_are_refused(weights):
    """2 S <= VNECT_MAX_SCALES: ten images do not fit the per-image tables; the handle without the batch setting still finalizes."""
    from vnect_amd import _native
    five = [1.0, 0.9, 0.8, 0.7, 0.6]
    with pytest.raises(_native.VnectError) as e:
        _native.Handle(five, stream_batch=2)
    assert e.value.code == _native.E_ARG and "VNECT_MAX_SCALES" in str(e.value)
    _make(weights, five).close()


@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_batched_plan_keeps_every_layer_of_the_scale_plan(weights, prec):
    scales = [1.0, 0.8, 0.6]
    plain = _make(weights, scales, precision=PRECISIONS[prec])
    h = _make(weights, scales, precision=PRECISIONS[prec], stream_batch=2)
    single, batched = h.layers(), h.batch_layers()
    assert single == plain.layers()                       # the handle's own plan does not change
    assert [L["name"] for L in batched] == [L["name"] for L in single]
    assert not any(L["name"] == "res5c_bone_length" for L in batched)
    assert any(">" in L["name"] for L in batched) and any("bone_length" in L["name"] for L in batched)   # the fused forms stay
    for a, b in zip(single, batched):
        assert (b["tile_m"], b["tile_n"], b["split_k"], b["N"], b["K"]) == (a["tile_m"], a["tile_n"], a["split_k"], a["N"], a["K"]), a["name"]
        assert b["M"] == 2 * a["M"], a["name"]
    with pytest.raises(Exception):
        plain.batch_layers()


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_batches_three_deep_on_three_lanes(weights, prec):
    scales = [1.0, 0.8, 0.6]
    n = 9
    vids, times = _videos(n), _times(n)
    want = _own(weights, scales, PRECISIONS[prec], vids[:2], times[:2])
    h = _make(weights, scales, precision=PRECISIONS[prec], stream_batch=2, lanes=3)
    got, inflight = [[], []], 0
    for k in range(n):
        if inflight == 3:
            for s in (0, 1):
                rs, j2, j3 = h.collect_stream()
                assert rs == s
                got[s].append((j2, j3))
            inflight -= 1
        sa, sb = (2 * k) % 8, (2 * k + 1) % 8
        h.upload_frame(sa, vids[0][k])
        h.upload_frame(sb, vids[1][k])
        h.submit_streams([0, 1], [sa, sb], [times[0][k], times[1][k]], [times[0][k] + 0.0005, times[1][k] + 0.0005])
        inflight += 1
    for _ in range(2 * inflight):
        rs, j2, j3 = h.collect_stream()
        got[rs].append((j2, j3))
    for s in (0, 1):
        assert len(got[s]) == n and all(_same(got[s][k], want[s][k]) for k in range(n)), s


def test_refused_batches_change_nothing(weights):
    from vnect_amd import _native
    scales = [1.0, 0.8]
    n = 4
    vids, times = _videos(n), _times(n)
    want = _own(weights, scales, 1, vids[:2], times[:2])
    # no batch setting: a batch of two is refused; the setting after finalize too
    plain = _make(weights, scales, precision=1)
    plain.upload_frame(0, vids[0][0])
    plain.upload_frame(1, vids[1][0])
    with pytest.raises(_native.VnectError) as e:
        plain.submit_streams([0, 1], [0, 1], [T0, T0], [T0, T0])
    assert e.value.code == _native.E_STATE
    with pytest.raises(_native.VnectError) as e:
        plain.set_stream_batch(2)
    assert e.value.code == _native.E_STATE
    h = _make(weights, scales, precision=1, stream_batch=2)
    got = [[], []]

    def batch(k, t2=None):
        h.upload_frame(0, vids[0][k])
        h.upload_frame(1, vids[1][k])
        tb = times[1][k] if t2 is None else t2
        h.submit_streams([0, 1], [0, 1], [times[0][k], tb], [times[0][k] + 0.0005, tb + 0.0005])
        for s in (0, 1):
            rs, j2, j3 = h.collect_stream()
            got[rs].append((j2, j3))

    def refused(code, *args):
        with pytest.raises(_native.VnectError) as e:
            h.submit_streams(*args)
        assert e.value.code == code, e.value

    batch(0)
    refused(_native.E_ARG, [1, 1], [0, 1], [times[0][1], times[1][1]], [times[0][1], times[1][1]])              # duplicate stream
    refused(_native.E_ARG, [0, 1, 2], [0, 1, 2], [times[0][1]] * 3, [times[0][1]] * 3)                         # n = 3
    refused(_native.E_TIMESTAMP, [0, 1], [0, 1], [times[0][1], times[1][0]], [times[0][1] + 0.0005, times[1][0] + 0.0005])  # stream 1 repeats
    refused(_native.E_ARG, [0, 1], [0, 5], [times[0][1], times[1][1]], [times[0][1], times[1][1]])              # empty slot
    batch(1)
    batch(2)
    refused(_native.E_TIMEORDER, [0, 1], [0, 1], [times[0][3], times[1][1]], [times[0][3] + 0.0005, times[1][1] + 0.0005])
    batch(3)
    for s in (0, 1):
        assert len(got[s]) == n and all(_same(got[s][k], want[s][k]) for k in range(n)), s
