"""Child process of tests/test_gpu_overlay.py: `python -m tests.overlay_torch_child`.

torch is imported BEFORE vnect_amd, so the process holds one HIP runtime.  VNectEstimator.draw on uint8 CUDA tensors of every layout -- packed,
a permuted CHW tensor, bgra[..., :3], a slice of a larger tensor, a transposed view, RGB order, NV12 in one tensor and as a (y, uv) pair --
must leave exactly the pixels render.draw_limbs_2d_exact (NV12: tests/overlay_ref.py) draws into the tensor's host copy, in the tensor's
WHOLE storage: the bytes around a view (the alpha bytes, the rest of the larger tensor) must be untouched.  A draw behind a write on a side
stream is ordered behind it.  The last line printed is `overlay child ok`; any failure is an assertion (exit status 1)."""
import numpy as np


def main():
    import torch
    from tests import overlay_ref as R
    from vnect_amd import VNectEstimator, render
    from vnect_amd.weights import synthetic_weights
    g = torch.Generator().manual_seed(11)
    H, W = 96, 128

    def rnd(*shape):
        return torch.randint(64, 128, shape, generator=g, dtype=torch.uint8).cuda()

    case = [c for c in R.cases(H, W) if c["name"] == "skeleton"][0]
    j2, parents, rect, conf, thr = case["joints"], case["parents"], case["rect"], case["conf"], case["thr"]
    assert parents == VNectEstimator.joint_parents
    est = VNectEstimator(weights=synthetic_weights(), verbose=False)
    try:
        chw, bgra, big, wh3 = rnd(3, H, W), rnd(H, W, 4), rnd(H + 20, W + 30, 3), rnd(W, H, 3)
        views = [("packed", rnd(H, W, 3), None, "bgr"), ("chw.permute(1, 2, 0)", chw, chw.permute(1, 2, 0), "bgr"),
                 ("bgra[..., :3]", bgra, bgra[..., :3], "bgr"), ("slice", big, big[7:7 + H, 11:11 + W], "rgb"),
                 ("transposed", wh3, wh3.permute(1, 0, 2), "bgr"), ("packed rgb", rnd(H, W, 3), None, "rgb")]
        for k, (name, store, v, fmt) in enumerate(views):
            v = store if v is None else v
            host_store = store.cpu().numpy().copy()
            # the same view of the host copy: same offset and strides (uint8: strides are bytes)
            off = v.storage_offset() - store.storage_offset()
            host_view = np.lib.stride_tricks.as_strided(host_store.reshape(-1)[off:], shape=tuple(v.shape), strides=tuple(v.stride()))
            kw = dict(confidence=conf, min_confidence=thr) if k % 2 else {}
            render.draw_limbs_2d_exact(host_view, j2, parents, rect, pixel_format=fmt, inplace=True, **kw)
            assert (host_store != store.cpu().numpy()).any(), name
            out = est.draw(v, j2, rect=rect, pixel_format=fmt, **kw)
            assert out is v and np.array_equal(store.cpu().numpy(), host_store), name
        # NV12: one (H * 3 // 2, W) tensor, and a (y, uv) pair with pitches of their own
        lay = dict(format=2, H=H, W=W, data_off=0, uv_off=H * W, sy=W, sx=1, sc=0, uv_stride=W, size=H * W * 3 // 2)
        nv = rnd(H * 3 // 2, W)
        want = nv.cpu().numpy().reshape(-1).copy()
        assert R.draw(want, lay, case) > 0
        est.draw(nv, j2, rect=rect, pixel_format="nv12", confidence=conf, min_confidence=thr)
        assert np.array_equal(nv.cpu().numpy().reshape(-1), want), "nv12"
        ys, us = rnd(H, W + 6), rnd(H // 2, W + 10)
        ywant, uwant = ys.cpu().numpy().copy(), us.cpu().numpy().copy()
        both = np.concatenate([ywant.reshape(-1), uwant.reshape(-1)])
        lay2 = dict(format=2, H=H, W=W, data_off=0, uv_off=ywant.size, sy=W + 6, sx=1, sc=0, uv_stride=W + 10, size=both.size)
        R.draw(both, lay2, dict(case, name="skeleton_pair", conf=None, thr=None), (10, 200, 30), (200, 10, 90))
        est.draw((ys[:, :W], us[:, :W]), j2, rect=rect, pixel_format="nv12", colors=((10, 200, 30), (200, 10, 90)))
        assert np.array_equal(np.concatenate([ys.cpu().numpy().reshape(-1), us.cpu().numpy().reshape(-1)]), both), "nv12 pair"
        # a target written on a side stream is drawn into behind that stream's work (stream= defaults to torch's current stream)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            t += 77
            est.draw(t, j2, rect=rect)
        want = render.draw_limbs_2d_exact(np.full((H, W, 3), 77, np.uint8), j2, parents, rect)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), want), "side stream"
    finally:
        est.close()
    print("overlay child ok")


if __name__ == "__main__":
    main()
