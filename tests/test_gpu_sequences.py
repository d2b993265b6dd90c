"""Sequence tensors on the GPU (lcfe_sequences_device through DeviceBatch.sequences): the fixture of
tests/test_sequences_cpu.py against the host build of the same template and against the tensors recorded from the
reference's module, objects extracted alone, max_length 8 against 500, an augmented batch against its re-staged rows, the
argument checks and the purity of the call.

Bounds: those of tests/test_sequences_cpu.py.  Device against host build: flux_mean / flux_std within 1 float32 ulp (64 lanes
add in another order than one), every other output bit-equal to the restatement's expressions evaluated with the device's own
flux_mean / flux_std -- and bit-equal to the host build outright for every object whose two statistics agree.
"""
import ctypes

import numpy as np
import pytest

import sequence_oracle as so
import test_augment_cpu as aug_cpu
import test_sequences_cpu as cpu
from test_sequences_cpu import golden, host, inputs, oracle  # noqa: F401  (fixtures)
from mallorn_astrophysics_amd import _lib
from mallorn_astrophysics_amd.augment import AugmentPlan
from mallorn_astrophysics_amd.engine import DeviceBatch

pytestmark = pytest.mark.gpu
KEYS = cpu.KEYS


def to_host(tensors):
    return {k: v.cpu().numpy() for k, v in tensors.items()}


@pytest.fixture(scope="module")
def device(inputs):  # noqa: F811
    """The fixture's batch and its tensors for every recorded setting, computed once."""
    batch = DeviceBatch(cpu.csr_of(inputs))
    return batch, {(L, norm): to_host(batch.sequences(L, norm)) for L, norm in cpu.SETTINGS}


@pytest.mark.parametrize("L,norm", cpu.SETTINGS)
def test_device_follows_host_build_and_reference(inputs, golden, oracle, host, device, L, norm):  # noqa: F811
    csr, got = cpu.csr_of(inputs), device[1][(L, norm)]
    for k, dt in (("features", np.float32), ("bands", np.int64), ("mask", np.float32), ("length", np.int64), ("flux_mean", np.float32),
                  ("flux_std", np.float32)):
        assert got[k].dtype == dt
    sim = cpu.host_sequences(host, csr, L, norm)
    for name in ("flux_mean", "flux_std"):
        assert (so.ulps(got[name], sim[name]) <= 1.0).all(), name
    cpu.assert_follows_oracle(got, csr, L, norm, oracle[(L, norm)], f"device L{L} normalize {norm}")
    same = (got["flux_mean"] == sim["flux_mean"]) & (got["flux_std"] == sim["flux_std"])
    print(f"statistics bit-equal to the host build for {int(same.sum())} of {same.size} objects")
    assert same.sum() >= same.size // 2
    for k in KEYS:
        assert np.array_equal(cpu.bits(got[k][same]), cpu.bits(sim[k][same])), k
    cpu.assert_matches_reference(got, inputs, golden, L, norm)


def test_object_alone_equals_its_row(inputs, device):  # noqa: F811
    csr, ids = cpu.csr_of(inputs), inputs["ids"].tolist()
    whole = device[1][(500, True)]
    for name in ("n1", "n501", "n2100"):
        i = ids.index(name)
        one = to_host(DeviceBatch(cpu.select(csr, [i])).sequences(500, True))
        for k in KEYS:
            assert np.array_equal(cpu.bits(one[k][0]), cpu.bits(whole[k][i])), (name, k)


def test_max_length_8_is_a_prefix_of_500(inputs, device):  # noqa: F811
    n = np.diff(inputs["offsets"])
    short = n <= 8
    assert short.sum() >= 5
    for norm in (True, False):
        a, b = device[1][(8, norm)], device[1][(500, norm)]
        for k in ("features", "bands", "mask"):
            assert np.array_equal(cpu.bits(a[k][short]), cpu.bits(b[k][short][:, :8])), k
        for k in ("length", "flux_mean", "flux_std"):
            assert np.array_equal(cpu.bits(a[k][short]), cpu.bits(b[k][short])), k
        # a truncated object keeps its times and its statistics: they are taken over all rows
        assert np.array_equal(cpu.bits(a["features"][~short]), cpu.bits(b["features"][~short][:, :8]))
        assert np.array_equal(cpu.bits(a["flux_std"]), cpu.bits(b["flux_std"]))


def test_augmented_batch_equals_its_restaged_rows():
    """The smallest plan of tests/test_gpu_augment.py's recipe, K = 2: objects of 0 to 700 rows, one out of time order,
    unknown filters, a NaN flux and a NaN time."""
    csr, k = aug_cpu.test_batch(), 2
    plan = AugmentPlan(len(aug_cpu.SIZES), k, **aug_cpu.mixed_plan(len(aug_cpu.SIZES), k))
    out = DeviceBatch(csr).augment(plan)
    got = to_host(out.sequences())
    rows = {"offsets": out.offsets.cpu().numpy(), "t": out.t.cpu().numpy(), "flux": out.flux.cpu().numpy(), "err": out.err.cpu().numpy(),
            "band": out.band.cpu().numpy()}
    want = to_host(DeviceBatch(rows).sequences())
    assert got["features"].shape == (k * len(aug_cpu.SIZES), 500, 4)
    for name in KEYS:
        assert got[name].tobytes() == want[name].tobytes(), name
    assert got["length"].tolist() == [max(1, min(500, int(n))) for n in np.diff(rows["offsets"])]


def test_bad_arguments_and_purity(inputs):  # noqa: F811
    import torch

    csr = cpu.csr_of(inputs)
    batch = DeviceBatch(csr)
    before = {k: getattr(batch, k).clone() for k in ("offsets", "t", "flux", "err", "band")}
    with pytest.raises(ValueError):
        batch.sequences(0)
    lib = _lib.load()
    out = batch.sequences(8)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    args = [p(getattr(batch, k)) for k in ("offsets", "t", "flux", "err", "band")] + [p(out[k]) for k in KEYS]
    stream = ctypes.c_void_p(torch.cuda.current_stream(batch.device).cuda_stream)

    def call(max_length=8, null=()):
        a = [None if j in null else x for j, x in enumerate(args)]
        return lib.lcfe_sequences_device(batch.device.index, stream, batch.n_obj, batch.n_points, max_length, 1, *a, None, 0)

    for kwargs, text in (({"max_length": 0}, b"max_length"), ({"null": (0,)}, b"null offsets"), ({"null": (2,)}, b"null sample"),
                         ({"null": (5,)}, b"null output"), ({"null": (9,)}, b"null output")):
        assert call(**kwargs) != 0, kwargs
        assert text in lib.lcfe_last_error(), (kwargs, lib.lcfe_last_error())
    assert call() == 0
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(batch, k).view(torch.uint8), v.view(torch.uint8)), k
    for k, v in csr.items():
        assert getattr(batch, k).cpu().numpy().tobytes() == v.tobytes(), k
