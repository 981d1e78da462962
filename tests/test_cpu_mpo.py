"""MPO handle (simplett/src/mpo/mpo.rs:35-60) without a GPU: shape validation happens on the host before the device is touched,
and valid input fails loudly (no CPU fallback)."""
import ctypes

import numpy as np
import pytest


def _new(dims4, cores=None):
    import t4a_amd
    d = np.asarray(dims4, dtype=np.uintp).reshape(-1)
    n = len(dims4)
    if cores is None:
        cores = np.zeros(max(sum(int(np.prod(x)) for x in dims4), 1))
    h = ctypes.c_void_p()
    st = t4a_amd._lib.t4a_gpu_mpo_new(t4a_amd._p(d) if n else None, ctypes.c_size_t(n), t4a_amd._p(cores), ctypes.byref(h))
    if h:
        t4a_amd._lib.t4a_gpu_mpo_release(h)
    return st, t4a_amd.last_error_message()


@pytest.mark.parametrize("dims4, needle", [
    ([(2, 2, 2, 1)], "first tensor must have left_dim=1"),
    ([(1, 2, 2, 3)], "last tensor must have right_dim=1"),
    ([(1, 2, 2, 3), (3, 2, 2, 2)], "last tensor must have right_dim=1"),
    ([(1, 2, 2, 3), (4, 2, 2, 1)], "Bond shape mismatch at site 0: left tensor has right_dim=3, right tensor has left_dim=4"),
    ([(1, 2, 2, 2), (2, 2, 2, 5), (3, 2, 2, 1)], "Bond shape mismatch at site 1"),
    ([(1, 0, 2, 1)], "zero dimension"),
    ([(1, 2, 2, 3), (3, 2, 0, 1)], "zero dimension"),
])
def test_new_rejects_bad_shapes_before_the_device(dims4, needle):
    import t4a_amd
    st, msg = _new(dims4)
    assert st == t4a_amd.INVALID_ARGUMENT, (st, msg)
    assert needle in msg


def test_new_rejects_sites_beyond_int_indexing():
    import t4a_amd
    # 1 x 65535 x 65535 x 1 elements > INT_MAX: refused by the shape check, no allocation and no device call
    st, msg = _new([(1, 65535, 65535, 1)], cores=np.zeros(1))
    assert st == t4a_amd.INVALID_ARGUMENT and "INT_MAX" in msg


def test_python_constructor_checks_the_leg_count():
    import t4a_amd
    with pytest.raises(t4a_amd.T4aError) as e:
        t4a_amd.MPO([np.ones((1, 2, 1))])
    assert e.value.code == t4a_amd.INVALID_ARGUMENT


def test_valid_mpo_without_gpu_is_no_device():
    import t4a_amd
    if t4a_amd.device_count() > 0:
        pytest.skip("a GPU is visible: the loud-failure path is covered on the CPU builder")
    for call in (lambda: t4a_amd.MPO.identity([2, 2]), lambda: t4a_amd.MPO.constant([(2, 3)], 1.5), lambda: t4a_amd.MPO([])):
        with pytest.raises(t4a_amd.T4aError) as e:
            call()
        assert e.value.code == t4a_amd.NO_DEVICE and "no CPU fallback" in e.value.message


def test_contraction_constants_match_the_header():
    import t4a_amd
    assert (t4a_amd.ContractionAlgorithm.Naive, t4a_amd.ContractionAlgorithm.ZipUp, t4a_amd.ContractionAlgorithm.Fit) == (0, 1, 2)
    assert (t4a_amd.FactorizeMethod.SVD, t4a_amd.FactorizeMethod.RSVD, t4a_amd.FactorizeMethod.LU, t4a_amd.FactorizeMethod.CI) == (0, 1, 2, 3)
    o = t4a_amd.ContractionOptions()
    assert o.tolerance == 1e-12 and o.max_bond_dim is None and o.factorize_method == t4a_amd.FactorizeMethod.SVD
