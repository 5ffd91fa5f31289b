"""Child process of tests/test_gpu_view3d.py: `python -m tests.view3d_torch_child`.

torch is imported BEFORE vnect_amd, so the process holds one HIP runtime.  VNectEstimator.view3d into a uint8 CUDA tensor, into a
row-pitched slice of one, and into the right-hand block of a canvas tensor whose left block VNectEstimator.preview filled must give exactly
render.view3d_exact, and must leave every other byte of the tensors' storage as it was.  The last line printed is `view3d child ok`; any
failure is an assertion (exit status 1)."""
import numpy as np


def main():
    import torch
    from tests import preview_ref as P
    from tests import view3d_ref as V
    from vnect_amd import VNectEstimator, render
    from vnect_amd.weights import synthetic_weights
    g = torch.Generator().manual_seed(5)
    est = VNectEstimator(weights=synthetic_weights(), verbose=False)
    try:
        j = V.skeleton(33)
        want = render.view3d_exact(j, (96, 130), order=1)
        assert (want != 255).any() and np.array_equal(want, V.view(j, 96, 130, order=1))
        out = torch.full((96, 130, 3), 0xA5, dtype=torch.uint8, device="cuda")
        assert est.view3d(j, (96, 130), out=out, order=1) is out
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(est.view3d(j, (96, 130), order=1), want)                    # and to a fresh numpy array
        # one canvas: the preview on the left, the view on the right, a margin of two columns between and behind them
        H, W = 96, 64
        frame = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
        case = P.skeleton(H, W)
        pv = render.preview_exact(frame.cpu().numpy(), case["joints"], case["parents"], case["rect"], factor=1.0)
        canvas = torch.full((H, W + 2 + H + 2, 3), 0xA5, dtype=torch.uint8, device="cuda")
        left, right = canvas[:, :W], canvas[:, W + 2:W + 2 + H]
        assert est.preview(frame, case["joints"], rect=case["rect"], factor=1.0, out=left) is left
        assert est.view3d(j, H, out=right, out_format="rgb") is right
        torch.cuda.synchronize()
        c = canvas.cpu().numpy()
        assert np.array_equal(c[:, :W], pv) and np.array_equal(c[:, W + 2:W + 2 + H], render.view3d_exact(j, H, out_format="rgb"))
        assert (c[:, W:W + 2] == 0xA5).all() and (c[:, W + 2 + H:] == 0xA5).all()
        for bad in (canvas[:, :W], canvas.permute(1, 0, 2)[:H, :H]):
            try:
                est.view3d(j, H, out=bad)
            except ValueError:
                continue
            raise AssertionError("a wrong `out` was accepted")
    finally:
        est.close()
    print("view3d child ok")


if __name__ == "__main__":
    main()
