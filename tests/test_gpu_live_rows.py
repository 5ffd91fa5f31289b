"""GPU (MI355X), through the C ABI: the live-rows mode of res2c's tail launch (rt_plan.cpp mark_live_rows, conv.hip live_fill).

res2c is read by res3a's two stride-2 1x1 convs only, so an arena plan's res2c_branch2b>res2c_branch2c computes the even pixels of the
92 x 92 grid and nothing else.  Every element it does compute sums the products the full launch sums, in its order, so everything behind
it is bit-identical: held here (a) on arena handles, by the joints of 8 frames with the mode on and off (VNECT_NO_LIVE_ROWS=1), and
(b) on the VNECT_KEEP_FUSED seam, where VNECT_FORCE_LIVE_ROWS=1 turns the mode on over private, zeroed buffers: res2c equal at the even
pixels and still zero everywhere else, res3a's two inputs and the final maps equal everywhere.  One scale is the smallest shape that can
go wrong: M = 8 464 has 2 116 live rows = 33 tiles of 64 and one of 4 (rows past the live count).  Both res2c wirings; the profiling twin;
the batched plan of two streams (2 S images); the recorded plan unchanged and rows_computed as specified (vnect_get_layer_rows)."""
import numpy as np
import pytest

from tests.gpu_common import BASELINE_SCALES, T0, _handle, _native

pytestmark = pytest.mark.gpu

SCALES = {1: [1.0], 2: [1.0, 0.7], 3: BASELINE_SCALES}
RES2C, RES3D = "res2c_branch2b>res2c_branch2c", "res3d_branch2b>res3d_branch2c"
CASES = [(1, False), (2, False), (3, False), (1, True), (3, True)]
IDS = ["S%d_%s" % (S, "paper" if p else "default") for S, p in CASES]


def _with_env(monkeypatch, env, *a, **kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return _handle(*a, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _plan(layers):
    return [(L["name"], L["tile_m"], L["tile_n"], L["split_k"], L["M"], L["N"], L["K"], L["workgroups"]) for L in layers]


def _frames(n, seed):
    from tests import helpers
    return [helpers.synth_frame(seed + k, 368, 300 + 17 * (k % 3), smooth=True) for k in range(n)]


def _check_rows(h, images, live, batch=False):
    """rows_computed: the live count for res2c's launch where the mode is on, M for every other launch; the rule's answer per launch"""
    layers = h.batch_layers() if batch else h.layers()
    rows = h.layer_rows(batch=batch)
    assert len(rows) == len(layers)
    names = [L["name"] for L in layers]
    assert names.count(RES2C) == 1
    for L, (computed, rule) in zip(layers, rows):
        if L["name"] == RES2C:
            assert L["M"] == images * 92 * 92 and L["workgroups"] == -(-L["M"] // 64) and (L["tile_m"], L["tile_n"]) == (64, 64)
            assert rule == 2 and computed == (images * 46 * 46 if live else L["M"]), (L, computed, rule)
        else:
            assert computed == L["M"] and rule == (2 if L["name"] == RES3D else 0), (L, computed, rule)


@pytest.mark.parametrize("S,paper", CASES, ids=IDS)
def test_arena_joints_are_equal_with_the_mode_on_and_off(weights, monkeypatch, S, paper):
    on = _handle(SCALES[S], weights, paper_res2c=paper)
    off = _with_env(monkeypatch, {"VNECT_NO_LIVE_ROWS": "1"}, SCALES[S], weights, paper_res2c=paper)
    try:
        assert _plan(on.layers()) == _plan(off.layers())   # every recorded field
        _check_rows(on, S, True)
        _check_rows(off, S, False)
        # flops count computed rows: res2c's launch does a quarter of its work
        f_on = {L["name"]: L["flops"] for L in on.layers()}
        f_off = {L["name"]: L["flops"] for L in off.layers()}
        assert f_on[RES2C] == f_off[RES2C] / 4 and all(f_on[n] == f_off[n] for n in f_on if n != RES2C)
        assert abs(on.timings()["conv_flops"] - (off.timings()["conv_flops"] - 0.75 * f_off[RES2C])) <= 1e-9 * off.timings()["conv_flops"]
        for k, fr in enumerate(_frames(8, 7300 + 10 * S)):
            t = T0 + 0.033 * k
            a, b = on.infer(fr, t, t + 0.0005), off.infer(fr, t, t + 0.0005)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (S, paper, k)
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("S,paper", CASES, ids=IDS)
def test_seam_computes_the_even_pixels_and_nothing_else(weights, monkeypatch, S, paper):
    import oracle
    from tests import helpers
    kw = dict(keep_activations=True, paper_res2c=paper)
    live = _with_env(monkeypatch, {"VNECT_KEEP_FUSED": "1", "VNECT_FORCE_LIVE_ROWS": "1"}, SCALES[S], weights, **kw)
    plain = _with_env(monkeypatch, {"VNECT_KEEP_FUSED": "1"}, SCALES[S], weights, **kw)   # the seam alone never takes the mode
    try:
        assert _plan(live.layers()) == _plan(plain.layers())
        _check_rows(live, S, True)
        _check_rows(plain, S, False)
        batch, _, _ = oracle.gen_input_batch(helpers.synth_frame(4321 + S, smooth=True), SCALES[S])
        out_l, out_p = live.forward(batch), plain.forward(batch)
        a, b = live.activation("res2c"), plain.activation("res2c")
        assert a.shape == b.shape == (S, 92, 92, 256) and float(np.abs(b).max()) > 0
        assert np.array_equal(a[:, ::2, ::2], b[:, ::2, ::2])
        dead = np.ones((92, 92), bool)
        dead[::2, ::2] = False
        assert not a[:, dead].any()           # never written: the buffer's zeros
        assert b[:, dead].any()               # (the full launch does write them)
        for name in ("res2b", "res3a_branch2a", "res3a_branch1", "res3a", "res3d", "res5c_branch2c"):
            assert np.array_equal(live.activation(name), plain.activation(name)), name
        assert np.array_equal(out_l, out_p)
        fr = helpers.synth_frame(77 + S, 368, 300, smooth=True)
        jl, jp = live.infer(fr, T0 + 5, T0 + 5.001), plain.infer(fr, T0 + 5, T0 + 5.001)
        assert np.array_equal(jl[0], jp[0]) and np.array_equal(jl[1], jp[1])
        a = live.activation("res2c")
        assert not a[:, dead].any() and np.array_equal(a[:, ::2, ::2], plain.activation("res2c")[:, ::2, ::2])
    finally:
        live.close()
        plain.close()


@pytest.mark.parametrize("S", [1, 3])
def test_profiling_twin_runs_with_the_mode_on(weights, monkeypatch, S):
    on = _handle(SCALES[S], weights)
    off = _with_env(monkeypatch, {"VNECT_NO_LIVE_ROWS": "1"}, SCALES[S], weights)
    try:
        on.set_profiling(True)
        for k, fr in enumerate(_frames(3, 7500 + S)):
            t = T0 + 0.033 * k
            a, b = on.infer(fr, t, t + 0.0005), off.infer(fr, t, t + 0.0005)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (S, k)
        ms = {L["name"]: L["last_ms"] for L in on.layers()}
        assert 0 < ms[RES2C] < 1.0 and on.timings()["frames"] == 3
        _check_rows(on, S, True)
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("S", [1, 2])
def test_batched_plan_of_two_streams_takes_the_mode(weights, monkeypatch, S):
    from tests import helpers
    x = np.stack([helpers.synth_frame(9600 + i, smooth=True).astype(np.float32) / 255.0 - 0.4 for i in range(2 * S)])
    on = _handle(SCALES[S], weights, stream_batch=2)
    off = _with_env(monkeypatch, {"VNECT_NO_LIVE_ROWS": "1"}, SCALES[S], weights, stream_batch=2)
    try:
        _check_rows(on, 2 * S, True, batch=True)
        _check_rows(off, 2 * S, False, batch=True)
        assert _plan(on.batch_layers()) == _plan(off.batch_layers())
        a, b = on.forward(x), off.forward(x)
        assert a.shape == (2 * S, 46, 46, 84) and np.array_equal(a, b)
    finally:
        on.close()
        off.close()


def test_forms_without_the_mode_keep_all_rows(weights, monkeypatch):
    """the 16-bit formats (chained and staged forms of the res2 stage) and the split-product handle leave the launch as it was; so does a
    keep_activations handle, with and without the seam, and VNECT_FORCE_LIVE_ROWS alone turns nothing on outside the seam"""
    n = _native()
    for prec in (n.BF16, n.FP16, n.FP32_SPLIT):
        h = _handle(SCALES[1], weights, precision=prec)
        try:
            rows = h.layer_rows()
            assert [r[0] for r in rows] == [L["M"] for L in h.layers()], prec
        finally:
            h.close()
    h = _with_env(monkeypatch, {"VNECT_FORCE_LIVE_ROWS": "1"}, SCALES[1], weights, keep_activations=True)
    try:
        assert [r[0] for r in h.layer_rows()] == [L["M"] for L in h.layers()] and not any(">" in L["name"] for L in h.layers())
    finally:
        h.close()
