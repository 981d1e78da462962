"""Host-only checks of compress_many (t4a_amd.mpo): the plan — routes at the bound of the batched kernels and one above it, the bounded
bond profiles, the launch and synchronisation counts — every refusal that needs no device with its message, the new symbols of the C
ABI, and the GAP CONDITION of every case tests/test_gpu_compress_many.py uses: at every cut of the restatement (tests/pmpo_np.py)
the kept singular values are >= 1e3 * cutoff and the dropped ones <= 1e-3 * cutoff, or the cut is made by the cap between values a
factor >= 1e3 apart, so that a rank can not hang on a rounding.  No device is touched."""
import os
import re

import numpy as np
import pytest
# This file is collected before tests/test_cpu_parallel.py and loads libt4a_gpu.so when it is imported: torch has to come first, as in
# tests/test_gpu_parallel.py (PyTorch-ROCm ships its own HIP runtime, and the first runtime a process loads serves it: INTEGRATION.md §4)
import torch  # noqa: F401

import t4a_amd
from t4a_amd import T4aError, INVALID_ARGUMENT
from t4a_amd import mpo as M
from t4a_amd.mpo import ContractionOptions, compress_many, compress_many_plan

import compress_many_np as H
import pmpo_np as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain(site_dims, bonds):
    return [(bonds[i], s1, s2, bonds[i + 1]) for i, (s1, s2) in enumerate(site_dims)]


# ------------------------------------------------------------------------------------------------ the plan
def test_bmax_is_64_and_the_routes_turn_at_it():
    assert M.COMPRESS_MANY_BMAX == 64 and H.BMAX == 64
    at = chain([H.E8, H.E8], [1, 64, 1])
    above = chain([H.E9, H.E9], [1, 65, 1])
    p = compress_many_plan([at, above, at], route="batched")
    assert p["routes"] == ["batched", "serial", "batched"] and p["n_batched"] == 2
    assert p["qr_bonds"] == [[1, 64, 1], [1, 65, 1], [1, 64, 1]]
    # the envelope is about the bond AFTER the shape-only bound of the right sweep: an input bond of 1000 that the QR bounds by 64 is in
    p = compress_many_plan([chain([H.E8, H.E8], [1, 1000, 1]), chain([H.E9, H.E9], [1, 1000, 1])], route="batched")
    assert p["routes"] == ["batched", "serial"] and p["qr_bonds"] == [[1, 64, 1], [1, 72, 1]]
    # one bond above the bound anywhere in the chain sends the item to the serial stage
    sd5 = [H.C] * 5
    assert compress_many_plan([chain(sd5, [1, 5, 64, 33, 5, 1])], route="batched")["routes"] == ["batched"]
    assert compress_many_plan([chain(sd5, [1, 5, 65, 33, 5, 1])], route="batched")["routes"] == ["serial"]


def test_bounded_profiles_with_the_wide_left_end_and_a_binding_cap():
    # the DESIGN.md case in small: binary legs, product bond 64 everywhere; the right sweep bounds the right end by the site dims, the
    # way back bounds the left end — the first left step is the wide 4 x 64 matrix
    n = 6
    shapes = chain([(2, 2)] * n, [1] + [64] * (n - 1) + [1])
    p = compress_many_plan([shapes], route="batched")
    assert p["qr_bonds"] == [[1, 64, 64, 64, 16, 4, 1]]
    assert p["bonds"] == [[1, 4, 16, 64, 16, 4, 1]]
    assert p["routes"] == ["batched"]
    capped = compress_many_plan([shapes], ContractionOptions(1e-12, 5), route="batched")
    assert capped["bonds"] == [[1, 4, 5, 5, 5, 4, 1]] and capped["qr_bonds"] == p["qr_bonds"]
    # the helper's own bounds are the same rule
    for n_sites in H.LENGTHS:
        for name in H.KIND_ORDER:
            sd, bonds, _ = H.KINDS[n_sites][name]
            for _, cap in H.OPTIONS:
                q = compress_many_plan([chain(sd, bonds)], ContractionOptions(1e-8, cap), route="batched")
                assert q["qr_bonds"] == [H.qr_bonds(chain(sd, bonds))] and q["bonds"] == [H.bound_bonds(chain(sd, bonds), cap)]
                assert q["routes"] == ["batched" if H.inside(chain(sd, bonds)) else "serial"]


def test_launches_and_syncs_do_not_depend_on_the_batch_size():
    for n_sites in (2, 3, 5, 12):
        one = chain([(2, 2)] * n_sites, [1] + [8] * (n_sites - 1) + [1])
        for count in (1, 3, 300):
            p = compress_many_plan([one] * count, route="batched")
            assert (p["launches"], p["syncs"], p["n_batched"]) == (2 * (n_sites - 1), 1, count)
    # nothing batched: nothing launched by the batched part
    p = compress_many_plan([chain([H.E9, H.E9], [1, 65, 1])] * 4, route="batched")
    assert (p["launches"], p["syncs"], p["n_batched"]) == (0, 0, 0)
    p = compress_many_plan([one] * 4, route="serial")
    assert (p["launches"], p["syncs"], p["n_batched"]) == (0, 0, 0) and p["routes"] == ["serial"] * 4
    # fewer than two sites: a copy
    p = compress_many_plan([[(1, 2, 2, 1)]] * 3, route="batched")
    assert p["routes"] == ["serial"] * 3 and p["launches"] == 0 and p["bonds"] == [[1, 1]] * 3


def test_auto_takes_the_kernels_for_small_bonds_and_from_sixteen_items_up():
    small = chain([(2, 2)] * 4, [1, 4, 16, 4, 1])
    large = chain([(2, 2)] * 4, [1, 4, 64, 4, 1])  # the QR bounds 64 by 16
    big = chain([H.E8, H.B, H.E8, H.B], [1, 64, 33, 4, 1])
    out = chain([H.E9, H.B, H.E9, H.E9], [1, 4, 4, 65, 1])
    assert compress_many_plan([large], route="auto")["qr_bonds"] == [[1, 4, 16, 4, 1]]
    # no bond above 16 after the right sweep: the kernels even for one item; an item outside the envelope stays serial
    assert compress_many_plan([small], route="auto")["routes"] == ["batched"]
    assert compress_many_plan([large, out, small], route="auto")["routes"] == ["batched", "serial", "batched"]
    # a bond above 16: the serial stage below 16 items inside the envelope, the kernels from 16 up
    assert compress_many_plan([big], route="auto")["qr_bonds"] == [[1, 64, 33, 4, 1]]
    assert compress_many_plan([big] * 15 + [out], route="auto")["routes"] == ["serial"] * 16
    assert compress_many_plan([small] * 14 + [big], route="auto")["routes"] == ["serial"] * 15
    assert compress_many_plan([big] * 16 + [out], route="auto")["routes"] == ["batched"] * 16 + ["serial"]
    assert compress_many_plan([big], route="batched")["routes"] == ["batched"]


# ------------------------------------------------------------------------------------------------ refusals
def refused(fn, message, code=INVALID_ARGUMENT):
    with pytest.raises(T4aError) as e:
        fn()
    assert e.value.code == code and e.value.message == message, e.value.message


def test_every_refusal_that_needs_no_device():
    one = chain([(2, 2)] * 3, [1, 4, 4, 1])
    refused(lambda: compress_many_plan([]), "compress_many: the list is empty")
    refused(lambda: compress_many([]), "compress_many: the list is empty")
    refused(lambda: compress_many_plan([one, one[:2] + [(4, 2, 2, 1)], one[:1] + [(4, 2, 2, 1)]]), "compress_many: item 2 has 2 sites, item 0 has 3")
    refused(lambda: compress_many_plan([one], route="fast"), "unknown compress route 'fast': one of 'auto', 'batched', 'serial'")
    refused(lambda: compress_many([], route="fast"), "unknown compress route 'fast': one of 'auto', 'batched', 'serial'")
    refused(lambda: compress_many([1, 2]), "compress_many: every item must be an MPO")
    refused(lambda: compress_many_plan([[(1, 2, 2)]]), "compress_many_plan: a site is (l, s1, s2, r)")
    # the shape checks of MPO(...) with the item in front
    refused(lambda: compress_many_plan([one, [(1, 2, 2, 4), (3, 2, 2, 4), (4, 2, 2, 1)]]),
            "compress_many: item 1: Bond shape mismatch at site 0: left tensor has right_dim=4, right tensor has left_dim=3")
    refused(lambda: compress_many_plan([[(2, 2, 2, 4), (4, 2, 2, 1)]]),
            "compress_many: item 0: Invalid boundary conditions: first tensor must have left_dim=1, last tensor must have right_dim=1")
    refused(lambda: compress_many_plan([[(1, 2, 0, 4), (4, 2, 2, 1)]]), "compress_many: item 0: MPO site 0 has a zero dimension")
    # the raw C ABI: an unknown route code and null arguments
    lib = t4a_amd._lib
    dims = np.array([1, 2, 2, 1], dtype=np.uintp)
    lens = np.array([1], dtype=np.uintp)
    args = (t4a_amd._p(dims), t4a_amd._p(lens), t4a_amd.c_size_t(1), t4a_amd.c_double(1e-12), t4a_amd.c_size_t(0))
    assert lib.t4a_gpu_mpo_compress_many_plan(*args, t4a_amd.c_int32(3), None, None, None, None) == INVALID_ARGUMENT
    assert lib.t4a_gpu_mpo_compress_many_plan(*args, t4a_amd.c_int32(1), None, None, None, None) == 0
    assert lib.t4a_gpu_mpo_compress_many_plan(None, None, t4a_amd.c_size_t(1), t4a_amd.c_double(1e-12), t4a_amd.c_size_t(0), t4a_amd.c_int32(1),
                                              None, None, None, None) == t4a_amd.NULL_POINTER
    out = (t4a_amd.c_void_p * 1)()
    assert lib.t4a_gpu_mpo_compress_many(None, t4a_amd.c_size_t(1), t4a_amd.c_double(1e-12), t4a_amd.c_size_t(0), t4a_amd.c_int32(1),
                                         out) == t4a_amd.NULL_POINTER
    null_item = (t4a_amd.c_void_p * 1)()
    assert lib.t4a_gpu_mpo_compress_many(null_item, t4a_amd.c_size_t(1), t4a_amd.c_double(1e-12), t4a_amd.c_size_t(0), t4a_amd.c_int32(1),
                                         out) == t4a_amd.NULL_POINTER
    assert t4a_amd.last_error_message() == "compress_many: item 0 is null" and not out[0]
    assert lib.t4a_gpu_mpo_compress(None, t4a_amd.c_double(1e-12), t4a_amd.c_size_t(0), out) == t4a_amd.NULL_POINTER


def test_the_c_abi_declares_and_exports_the_new_entry_points():
    with open(os.path.join(ROOT, "include", "t4a_gpu.h")) as f:
        header = f.read()
    for name in ("t4a_gpu_mpo_compress", "t4a_gpu_mpo_compress_many", "t4a_gpu_mpo_compress_many_counted", "t4a_gpu_mpo_compress_many_plan",
                 "t4a_gpu_mpo_time_compress_many", "t4a_gpu_pmpo_contract_routed", "t4a_gpu_pmpo_time_compress"):
        assert re.search(r"t4a_gpu_status\s+" + name + r"\(", header), name
        assert hasattr(t4a_amd._lib, name), name
    for name, value in (("T4A_GPU_COMPRESS_AUTO", 0), ("T4A_GPU_COMPRESS_BATCHED", 1), ("T4A_GPU_COMPRESS_SERIAL", 2),
                        ("T4A_GPU_COMPRESS_MANY_BMAX", 64)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", header), name
    assert M._ROUTES == {"auto": 0, "batched": 1, "serial": 2}


# ------------------------------------------------------------------------------------------------ the gap condition
@pytest.mark.parametrize("n_sites", H.LENGTHS)
def test_every_case_of_the_gpu_tests_has_a_gap_at_every_cut(n_sites):
    seen = set()
    for size in H.SIZES:
        names, items = H.batch(n_sites, size)
        assert len(items) == size
        for tol, cap in H.OPTIONS:
            for k, (name, item) in enumerate(zip(names, items)):
                report = H.cut_report(item, tol, cap)
                assert len(report) == n_sites - 1
                for i, cut in enumerate(report):
                    assert H.gap_ok(cut), (n_sites, size, k, name, tol, cap, i, cut)
                # the restatement's ranks are those of the report
                assert [t.shape[0] for t in P.compress(item, tol, cap)[1:]] == [c["rank"] for c in report]
                if size >= 11:
                    seen.update((name, o) for o in H.orientations(item, tol, cap))
    # what every batch of 300 holds: a tall, a square and a wide step, and the kinds by name
    assert {o for _, o in seen} == {"tall", "square", "wide"}
    assert {name for name, _ in seen} == set(H.KIND_ORDER)


@pytest.mark.parametrize("n_sites", H.LENGTHS)
def test_the_kinds_are_what_their_names_say(n_sites):
    names, items = H.batch(n_sites, 300)
    by = {}
    for name, item in zip(names, items):
        by.setdefault(name, item)
    assert H.orientations(by["tall"], 1e-8, None)[0] == "tall"
    assert H.orientations(by["square"], 1e-8, None)[0] == "square"
    assert H.orientations(by["wide"], 1e-8, None)[0] == "wide"
    assert all(t.shape[0] == 1 and t.shape[3] == 1 for t in by["bond1"])
    assert all(not t.any() for t in by["zero"]) and [c["rank"] for c in H.cut_report(by["zero"], 1e-8, None)] == [1] * (n_sites - 1)
    # cut to rank 1 by the tolerance although the bonds are larger
    assert [c["rank"] for c in H.cut_report(by["rank1"], 1e-8, None)] == [1] * (n_sites - 1) and max(t.shape[3] for t in by["rank1"]) >= 5
    # the tolerance binds at the first bond (values are dropped there, the rank stays under the cap), the cap at a later one
    rep = H.cut_report(by["tol_and_cap"], 1e-8, 2)
    if n_sites == 2:  # one bond: the cap binds with it, the tolerance without it
        assert rep[0]["by_cap"] and H.cut_report(by["tol_and_cap"], 1e-8, None)[0]["rank"] == 4
    else:
        assert rep[0]["rank"] == 1 and not rep[0]["by_cap"] and rep[0]["cols"] > 1 and rep[-1]["by_cap"] and rep[-1]["rank"] == 2
    assert max(H.qr_bonds(H.shapes_of(by["bmax"]))) == 64 and H.inside(H.shapes_of(by["bmax"]))
    assert max(H.qr_bonds(H.shapes_of(by["bmax_plus_1"]))) == 65 and not H.inside(H.shapes_of(by["bmax_plus_1"]))
    assert max(float(np.abs(t).max()) for t in by["big"]) > 1e118 and 0 < max(float(np.abs(t).max()) for t in by["small"][1:] + by["small"][:1])
    assert min(float(np.abs(t).max()) for t in by["small"]) < 1e-118
    # every site dim and bond comes from the lists of the issue (plus (8, 8) and (8, 9), which reach a bond of 64 and 65 at two and three sites)
    for name in H.KIND_ORDER:
        sd, bonds, _ = H.KINDS[n_sites][name]
        assert set(sd) <= {H.A, H.B, H.C, H.D, H.E8, H.E9} and set(bonds) <= {1, 2, 3, 5, 8, 15, 16, 17, 33, 64, 65}, name


@pytest.mark.parametrize("n, ys, xs, zs", H.PMPO_CASES)
def test_the_partitioned_cases_have_a_gap_at_every_cut(n, ys, xs, zs):
    real_cap_cuts = 0
    for tol, cap in H.PMPO_OPTIONS:
        products = H.pmpo_task_products(n, ys, xs, zs, cap)
        assert len(products) >= 2
        for t, item in enumerate(products):
            for i, cut in enumerate(H.cut_report(item, tol, cap)):
                assert H.gap_ok(cut), (n, ys, tol, cap, t, i, cut)
                # a cut the cap makes between two nonzero values, which the tolerance alone would both have kept
                real_cap_cuts += cut["by_cap"] and cut["dropped_max"] >= H.GAP * cut["cutoff"]
    assert real_cap_cuts >= 1


def test_the_items_are_what_the_docstring_promises():
    # a sum of orthogonal product operators: the singular values at a cut where both sides tell the terms apart are |COEFFS|
    item = H.make_item(7, [H.C, H.C, H.C], [1, 8, 8, 1])
    for cut in H.cut_report(item, 0.0, None):
        assert cut["rank"] == min(cut["rows"], cut["cols"])
    s = np.linalg.svd(P.full(item).reshape(6, 36), compute_uv=False)  # the cut behind site 0 of the dense operator [i1, j1, i2, j2, i3, j3]
    assert np.allclose(s[:4], np.abs(H.COEFFS), rtol=1e-12, atol=1e-15) and s[4] < 1e-15
    # seeded: the same item twice
    again = H.make_item(7, [H.C, H.C, H.C], [1, 8, 8, 1])
    assert all(np.array_equal(a, b) for a, b in zip(item, again))
