"""Child process of tests/test_gpu_preview.py: `python -m tests.preview_torch_child`.

torch is imported BEFORE vnect_amd, so the process holds one HIP runtime.  VNectEstimator.preview on uint8 CUDA tensors of every layout --
packed, a permuted CHW tensor, bgra[..., :3], a slice of a larger tensor, a transposed view, RGB order, NV12 in one tensor and as a (y, uv)
pair -- must return exactly render.preview_exact of the tensor's host copy, to a numpy array and into a torch `out` (also a row-pitched
one), and must leave the tensor's WHOLE storage as it was.  A preview behind a write on a side stream is ordered behind it.  The last line
printed is `preview child ok`; any failure is an assertion (exit status 1)."""
import numpy as np


def main():
    import torch
    from tests import nv12_ref
    from tests import preview_ref as P
    from vnect_amd import VNectEstimator, render
    from vnect_amd.weights import synthetic_weights
    g = torch.Generator().manual_seed(11)
    H, W = 96, 64

    def rnd(*shape):
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda()

    case = P.skeleton(H, W)
    j2, parents, rect = case["joints"], case["parents"], case["rect"]
    assert parents == VNectEstimator.joint_parents
    est = VNectEstimator(weights=synthetic_weights(), verbose=False)
    try:
        chw, bgra, big, wh3 = rnd(3, H, W), rnd(H, W, 4), rnd(H + 20, W + 30, 3), rnd(W, H, 3)
        views = [("packed", rnd(H, W, 3), None, "bgr"), ("chw.permute(1, 2, 0)", chw, chw.permute(1, 2, 0), "bgr"),
                 ("bgra[..., :3]", bgra, bgra[..., :3], "bgr"), ("slice", big, big[7:7 + H, 11:11 + W], "rgb"),
                 ("transposed", wh3, wh3.permute(1, 0, 2), "bgr"), ("packed rgb", rnd(H, W, 3), None, "rgb")]
        for k, (name, store, v, fmt) in enumerate(views):
            v = store if v is None else v
            before = store.cpu().numpy().copy()
            pic = v.cpu().numpy()
            pic = np.ascontiguousarray(pic[:, :, ::-1] if fmt == "rgb" else pic)
            f = P.FACTORS[k % len(P.FACTORS)]
            want = render.preview_exact(pic, j2, parents, rect, factor=f, out_format=("bgr", "rgb")[k % 2])
            got = est.preview(v, j2, rect=rect, pixel_format=fmt, factor=f, out_format=("bgr", "rgb")[k % 2])
            assert np.array_equal(got, want) and (want != render.preview_exact(pic, None, parents, None, factor=f, out_format=("bgr", "rgb")[k % 2])).any(), name
            wide = torch.full((want.shape[0], want.shape[1] + 3, 3), 0xA5, dtype=torch.uint8, device="cuda")
            out = wide[:, :want.shape[1]]                             # rows 9 bytes longer than the picture's
            assert est.preview(v, j2, rect=rect, pixel_format=fmt, factor=f, out=out, out_format=("bgr", "rgb")[k % 2]) is out
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want) and (wide[:, want.shape[1]:] == 0xA5).all().item(), name
            assert np.array_equal(store.cpu().numpy(), before), (name, "the source was written")
        # NV12: one (H * 3 // 2, W) tensor, and a (y, uv) pair with pitches of their own, under an orientation
        nv = rnd(H * 3 // 2, W)
        pic = nv12_ref.restate(nv.cpu().numpy())
        assert np.array_equal(est.preview(nv, j2, rect=rect, pixel_format="nv12", factor=0.5), render.preview_exact(pic, j2, parents, rect, factor=0.5)), "nv12"
        ys, us = rnd(H, W + 6), rnd(H // 2, W + 10)
        both = np.concatenate([ys[:, :W].cpu().numpy(), us[:, :W].cpu().numpy()])
        turned = np.ascontiguousarray(np.rot90(nv12_ref.restate(both), 3))
        c3 = P.skeleton(W, H)
        got = est.preview((ys[:, :W], us[:, :W]), c3["joints"], rect=c3["rect"], pixel_format="nv12", orientation=3)
        assert np.array_equal(got, render.preview_exact(turned, c3["joints"], parents, c3["rect"])), "nv12 pair, code 3"
        # a frame written on a side stream is read behind that stream's work (stream= defaults to torch's current stream)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            t += 77
            got = est.preview(t, j2, rect=rect, factor=1.7)
        assert np.array_equal(got, render.preview_exact(np.full((H, W, 3), 77, np.uint8), j2, parents, rect, factor=1.7)), "side stream"
    finally:
        est.close()
    print("preview child ok")


if __name__ == "__main__":
    main()
