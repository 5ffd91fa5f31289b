"""Child process of tests/test_gpu_device_frames.py: `python -m tests.devframe_torch_child torch_first | vnect_first`.

torch_first: torch is imported BEFORE vnect_amd, so the process holds one HIP runtime; est(tensor) on four kinds of uint8 CUDA tensors must
equal est(tensor.cpu().numpy()) made contiguous, bit for bit.  vnect_first: vnect_amd is imported and a handle opened first, torch
afterwards; with two runtimes mapped, est(tensor) must be refused with the import-order sentence (a ValueError; nothing is launched) -- or,
where torch's second runtime finds no GPU at all and so can make no tensor, a pointer this runtime never allocated must be -- and with
one runtime it must work.  The last line printed says which case applied; any failure is an assertion (exit status 1)."""
import sys

import numpy as np

T0 = 1.7e9


def _times(k):
    return (T0 + 0.033 * k + 0.002 * (k % 3), T0 + 0.033 * k + 0.0005)


def _tensors(torch):
    """(name, uint8 CUDA tensor of shape (H, W, 3) as the estimator sees it)"""
    g = torch.Generator().manual_seed(5)
    H, W = 96, 128
    packed = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    chw = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).cuda()
    bgra = torch.randint(0, 256, (H, W, 4), generator=g, dtype=torch.uint8).cuda()
    big = torch.randint(0, 256, (H + 20, W + 30, 3), generator=g, dtype=torch.uint8).cuda()
    return [("packed", packed), ("chw.permute(1, 2, 0)", chw.permute(1, 2, 0)), ("bgra[..., :3]", bgra[..., :3]), ("slice", big[7:7 + H, 11:11 + W])]


def _estimators(n):
    from vnect_amd import VNectEstimator
    from vnect_amd.weights import synthetic_weights
    w = synthetic_weights()
    return [VNectEstimator(weights=w, verbose=False) for _ in range(n)]


def torch_first():
    import torch
    from vnect_amd import _native
    a, b = _estimators(2)
    try:
        for k, (name, t) in enumerate(_tensors(torch)):
            got = a(t, timestamp=_times(k))
            want = b(np.ascontiguousarray(t.cpu().numpy()), timestamp=_times(k))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        # a tensor written on a side stream is read behind that stream's work (stream= defaults to torch's current stream)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.zeros((96, 128, 3), dtype=torch.uint8, device="cuda")
            t += 77
            got = a(t, timestamp=_times(10))
        want = b(np.full((96, 128, 3), 77, np.uint8), timestamp=_times(10))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "side stream"
    finally:
        a.close(), b.close()
    libs = _native.hip_runtimes_mapped()
    assert len(libs) == 1, libs
    print("one runtime:", libs[0])


def vnect_first():
    from vnect_amd import _native
    a, b = _estimators(2)
    try:
        import torch
        libs = _native.hip_runtimes_mapped()
        try:
            tensors = _tensors(torch)
        except RuntimeError as e:                      # the second runtime may find no GPU at all (the first holds it): torch's own error
            assert len(libs) > 1, (libs, e)
            tensors = None
        if tensors is None:
            # no tensor can exist on the GPU; what reaches the library from the other runtime's side is a pointer this one never allocated
            frame = np.zeros((96, 128, 3), np.uint8)
            from tests.devframe_ref import FakeCuda
            try:
                a(FakeCuda(frame.ctypes.data, frame.shape), timestamp=_times(0))
            except ValueError as e:
                assert isinstance(e, _native.VnectError) and e.code == _native.E_ARG and _native.IMPORT_ORDER_HINT in str(e), str(e)
            else:
                raise AssertionError("a pointer this runtime never allocated was not refused")
            got, want = a(frame, timestamp=_times(0)), b(frame, timestamp=_times(0))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            print("two runtimes: torch finds no GPU; a foreign pointer is refused with the import-order sentence", libs)
        elif len(libs) > 1:
            for k, (name, t) in enumerate(tensors):
                try:
                    a(t, timestamp=_times(k))
                except ValueError as e:
                    assert isinstance(e, _native.VnectError) and e.code == _native.E_ARG, (name, e)
                    assert _native.IMPORT_ORDER_HINT in str(e), (name, str(e))
                else:
                    raise AssertionError("two HIP runtimes, and est(%s) was not refused" % name)
            # nothing was committed: the host frame next gives what a handle that saw only it gives
            frame = np.ascontiguousarray(tensors[0][1].cpu().numpy())
            got, want = a(frame, timestamp=_times(0)), b(frame, timestamp=_times(0))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            print("two runtimes: refused with the import-order sentence", libs)
        else:
            for k, (name, t) in enumerate(tensors):
                got = a(t, timestamp=_times(k))
                want = b(np.ascontiguousarray(t.cpu().numpy()), timestamp=_times(k))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
            print("one runtime:", libs)
    finally:
        a.close(), b.close()


if __name__ == "__main__":
    {"torch_first": torch_first, "vnect_first": vnect_first}[sys.argv[1]]()
