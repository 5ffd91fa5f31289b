"""GPU: the preview kernel of preview.hip alone, byte for byte against the composition of existing pins (tests/preview_ref.py; PREVIEW.md).

The product's own preview.o, linked behind a test shim (`make previewprobe`: vnect_amd/csrc/preview_probe.hip; the product never loads
it), is driven case by case.  The source lies in a device buffer of its own (NV12 in two planes: in two), the output in a device buffer
with a guard zone in front of and behind it; afterwards the WHOLE output buffer -- rows, pitch padding, the bytes in front of the first
row -- must equal the reference's, both guards must still hold their canary, and the source must be byte-identical.  The cases, layouts,
codes and factors are those of tests/test_preview_cpu.py; the tile straddles are derived from the tile the probe reports.  No case is
skipped: one the shim refuses fails."""
import numpy as np
import pytest

from tests import orient_ref
from tests import preview_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    L = P.probe_lib()
    lay = np.zeros(6, np.int32)
    L.pp_layout(lay.ctypes.data_as(P.i32p))
    L.fill, L.guard = int(lay[0]), int(lay[1])
    assert tuple(int(v) for v in lay[2:6]) == P.tile()          # the probe and the CPU shim were built from one preview.h
    return L


@pytest.mark.parametrize("size", P.SIZES, ids=["%dx%d" % s for s in P.SIZES])
@pytest.mark.parametrize("layout", range(len(P.LAYOUT_NAMES)), ids=P.LAYOUT_NAMES)
def test_every_case_in_every_layout_equals_the_composition(probe, size, layout):
    shares = P.run_jobs(size, layout, P.make_gpu_backend(probe, probe.guard, probe.fill))
    assert shares
    for key, share in shares:
        assert 0.05 <= share <= 0.95, (key, share)


def test_footprints_defaults_thin_outputs_and_tile_straddles(probe):
    P.run_special(P.make_gpu_backend(probe, probe.guard, probe.fill))


@pytest.mark.parametrize("form", ["packed4", "planar", "transposed", "nv12_pitched_odd_base", "nv12_two_planes"])
def test_every_orientation_of_every_source_form(probe, form):
    size = P.SIZES[0]
    lay = [l for l in P.layouts(*size) if l["name"] == form][0]
    backend = P.make_gpu_backend(probe, probe.guard, probe.fill)
    src = P.fresh(lay)
    for o in range(8):
        Hp, Wp = orient_ref.oriented_size(o, lay["H"], lay["W"])
        case = P.skeleton(Hp, Wp)
        f = (0.5, 1.7)[o % 2]
        exp = P.expected(src, lay, o, case, f)
        out, pitch = P.out_buffer(exp.shape[0], exp.shape[1], o % 4, 3)
        after = backend(src.copy(), lay, o, case, f, 0, out, o % 4, pitch)
        assert np.array_equal(after, src) and np.array_equal(out, P.whole(exp, o % 4, pitch)), (form, o, f)


def test_the_tracked_form_reads_its_inputs_on_the_device(probe):
    """the same kernel with joints, rect, status and confidences in JointsOut / TrackOut / ConfOut structures in device memory, as a tracked
    submit would launch it; a status other than OK writes nothing"""
    size = P.SIZES[1]
    for lay in [l for l in P.layouts(*size) if l["name"] in ("packed3_padded", "nv12_pitched_odd_base")]:
        src = P.fresh(lay)
        for o in (0, 3):
            Hp, Wp = orient_ref.oriented_size(o, lay["H"], lay["W"])
            for case in [c for c in P.cases(Hp, Wp) if c["joints"] is not None and c.get("rect") is not None]:
                exp = P.expected(src, lay, o, case, 0.37, 1)
                out, pitch = P.out_buffer(exp.shape[0], exp.shape[1], 1, 2)
                P.make_gpu_backend(probe, probe.guard, probe.fill, tracked=1)(src.copy(), lay, o, case, 0.37, 1, out, 1, pitch)
                assert np.array_equal(out, P.whole(exp, 1, pitch)), (lay["name"], o, case["name"])
            case = P.skeleton(Hp, Wp)
            for status in (1, 2, 3):
                out, pitch = P.out_buffer(*P.shape_of(Hp, Wp, 0.5), 0, 0)
                P.make_gpu_backend(probe, probe.guard, probe.fill, tracked=1, status=status)(src.copy(), lay, o, case, 0.5, 0, out, 0, pitch)
                assert (out == P.CANARY).all(), (lay["name"], o, status)
