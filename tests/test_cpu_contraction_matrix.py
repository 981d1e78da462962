"""The device route of candidate matrices without a GPU: the new symbols are declared in the header and exported, NULL handles are refused
with INVALID_ARGUMENT before a device is touched, and the Python argument checks that need no handle."""
import ctypes
import inspect
import os

import numpy as np
import pytest

SYMBOLS = ["t4a_gpu_contraction_evaluate_matrix", "t4a_gpu_tci2_set_contraction_source", "t4a_gpu_tci2_source_stats",
           "t4a_gpu_mpo_contract_tci_device"]


def test_every_new_symbol_is_declared_and_exported():
    import t4a_amd
    lib = ctypes.CDLL(t4a_amd.LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t4a_gpu.h")).read()
    assert all(s + "(" in header for s in SYMBOLS)


def test_null_handles_answer_invalid_argument_before_the_device():
    import t4a_amd
    lib = t4a_amd._lib
    p = t4a_amd._p
    h = ctypes.c_void_p()
    buf = np.zeros(8)
    idx = np.zeros(8, dtype=np.uintp)
    stats = (ctypes.c_uint64 * 3)(7, 7, 7)
    o = t4a_amd.TCI2Options().to_c()
    one = ctypes.c_size_t(1)
    calls = {
        "evaluate_matrix": lambda: lib.t4a_gpu_contraction_evaluate_matrix(None, one, p(idx), one, p(idx), one, p(buf)),
        "set_contraction_source": lambda: lib.t4a_gpu_tci2_set_contraction_source(None, None),
        "source_stats": lambda: lib.t4a_gpu_tci2_source_stats(None, stats),
        "contract_tci_device": lambda: lib.t4a_gpu_mpo_contract_tci_device(None, None, ctypes.byref(o), None, ctypes.c_size_t(0),
                                                                           ctypes.byref(h), p(buf)),
        "contract_tci_device out": lambda: lib.t4a_gpu_mpo_contract_tci_device(None, None, ctypes.byref(o), None, ctypes.c_size_t(0), None,
                                                                               p(buf)),
    }
    for name, call in calls.items():
        assert call() == t4a_amd.INVALID_ARGUMENT, name
        assert "is null" in t4a_amd.last_error_message(), name
        assert not h, name
    assert list(stats) == [7, 7, 7] and not buf.any()


def test_the_route_is_checked_before_any_handle_is_used():
    import t4a_amd
    from t4a_amd.mpo import contract_tci
    for bad in ("gpu", "", None, 1):
        with pytest.raises(t4a_amd.T4aError) as e:
            contract_tci(None, None, route=bad)
        assert e.value.code == t4a_amd.INVALID_ARGUMENT and "unknown route" in e.value.message
    sig = inspect.signature(contract_tci)
    assert sig.parameters["route"].default == "host" and list(sig.parameters) == ["a", "b", "options", "initial_pivots", "route"]
    assert hasattr(t4a_amd.Contraction, "evaluate_matrix")
    assert hasattr(t4a_amd.TensorCI2, "set_contraction_source") and hasattr(t4a_amd.TensorCI2, "source_stats")
