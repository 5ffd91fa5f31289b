"""Child process of tests/test_gpu_people.py: `python -m tests.people_torch_child`.

torch is imported BEFORE vnect_amd, so the process holds one HIP runtime.  The frames of the people video are uint8 CUDA tensors WRITTEN ON A
SIDE STREAM right before the loop submits them (runner.track_people_on_device takes torch's current stream as each frame's producer): three
persons, paired, with draw and preview, must yield what runner.track yields per person over the host copies of the frames, the frame
afterwards must be the P host draws in order and the picture their scaled composition.  The last line printed is `people child ok`; any
failure is an assertion (exit status 1)."""
import numpy as np


def main():
    import torch
    from tests import test_gpu_people as T
    from vnect_amd import render, runner
    P = 3
    host = T._video(T.SMALL)
    want = T._reference("bf16", T.S3, T.SMALL, P)
    side = torch.cuda.Stream()
    tensors = []

    def frames():
        for f in host:                                       # (consumed under `with torch.cuda.stream(side)` below)
            t = torch.zeros(f.shape, dtype=torch.uint8, device="cuda")
            t += torch.from_numpy(f).cuda()                  # written on the side stream, which is current when the loop takes the frame
            tensors.append(t)
            yield t

    est = T._est(precision="bf16", scales=list(T.S3), people=P, pair_people=True, lanes=2)
    try:
        with torch.cuda.stream(side):
            got = list(runner.track_people_on_device(est, frames(), T._rects(T.SMALL, P), timestamps=T._times(), ahead=1, source="device",
                                                     confidence=True, draw=True, preview=0.5))
    finally:
        est.close()
    T._same(got, want, "torch child")
    torch.cuda.synchronize()
    for k, (people, picture) in enumerate(got):
        clean = host[k]
        drawn = clean
        for g in people:
            drawn = render.draw_limbs_2d_exact(drawn, g[0], est.joint_parents, list(g[2]))
        assert np.array_equal(tensors[k].cpu().numpy(), drawn), k
        assert np.array_equal(picture, render.resize_u8_exact(drawn, 0.5)), k
    print("people child ok")


if __name__ == "__main__":
    main()
