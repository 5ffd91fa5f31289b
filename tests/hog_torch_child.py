"""Child process of tests/test_gpu_hog.py: `python -m tests.hog_torch_child`.

torch is imported BEFORE vnect_amd, so the process holds one HIP runtime.  VNectEstimator.detect_people on uint8 CUDA tensors of every
layout -- packed, a permuted CHW tensor, bgra[..., :3], a slice of a larger tensor, RGB order, NV12 in one tensor -- must return exactly
the numpy statement's rects and weights (tests/hog_ref.py) over the tensor's host copy, and must leave the tensor's WHOLE storage as it
was.  A detection behind a write on a side stream is ordered behind it.  The last line printed is `hog child ok`; any failure is an
assertion (exit status 1)."""
import numpy as np


def main():
    import torch
    from tests import hog_ref as R
    from tests import nv12_ref
    from vnect_amd import VNectEstimator, runner
    from vnect_amd.weights import synthetic_weights
    H, W = 200, 104
    det = R.seeded_detector(1, rho=0.05, scale=0.04)
    spec = dict(final_threshold=0.5)                                  # the hits ungrouped: every window's score counts
    s = R.spec(**spec)

    def check(got, pic, name):
        ref = R.detect(pic, det, s, keep=False)
        assert ref["hits"], name
        assert [tuple(int(v) for v in r) for r in got[0]] == [tuple(r) for r in ref["rects"]], name
        assert np.array_equal(got[1], np.array(ref["weights"])), name

    est = VNectEstimator(scales=[1.0], weights=synthetic_weights(), verbose=False, hog_detector=det)
    try:
        pic = R.textured(H, W, seed=21)
        t = torch.from_numpy(pic).cuda()
        chw = torch.from_numpy(np.ascontiguousarray(pic.transpose(2, 0, 1))).cuda()
        bgra = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        bgra[..., :3] = t
        big = torch.zeros((H + 20, W + 30, 3), dtype=torch.uint8, device="cuda")
        big[7:7 + H, 11:11 + W] = t
        rgb = torch.from_numpy(np.ascontiguousarray(pic[:, :, ::-1])).cuda()
        views = [("packed", t, t, "bgr"), ("chw.permute(1, 2, 0)", chw, chw.permute(1, 2, 0), "bgr"), ("bgra[..., :3]", bgra, bgra[..., :3], "bgr"),
                 ("slice", big, big[7:7 + H, 11:11 + W], "bgr"), ("packed rgb", rgb, rgb, "rgb")]
        for name, store, v, fmt in views:
            before = store.cpu().numpy().copy()
            check(est.detect_people(v, pixel_format=fmt, **spec), pic, name)
            assert np.array_equal(store.cpu().numpy(), before), (name, "the source was written")
        g = torch.Generator().manual_seed(11)
        nv = torch.randint(0, 256, (H * 3 // 2, W), generator=g, dtype=torch.uint8).cuda()
        check(est.detect_people(nv, pixel_format="nv12", **spec), nv12_ref.restate(nv.cpu().numpy()), "nv12")
        turned = np.ascontiguousarray(np.rot90(pic, -3))
        check(est.detect_people(torch.from_numpy(turned).cuda(), orientation=3, **spec), pic, "code 3")
        assert runner.hog_box(est, t) == runner.hog_box(est, pic)
        # a frame written on a side stream is read behind that stream's work (stream= defaults to torch's current stream)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            z = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            z += t
            got = est.detect_people(z, **spec)
        check(got, pic, "side stream")
    finally:
        est.close()
    print("hog child ok")


if __name__ == "__main__":
    main()
