"""The launch caps of csrc/: every place where a launcher clamps its grid (or its threads) to 1024, 2048, 4096, 8192 or 65535 and leaves the
rest to a loop inside the kernel.  One row per clamp, as a source search finds them (find_clamps below: `std::min(..., N)`,
`if (x > N) x = N` and `x < N ? x : N`):

  file       the source under tensor4all-rs_amd/csrc
  launcher   the function whose body holds the clamp
  capped     what is clamped: "grid x", "grid y", or "threads" (of the one workgroup)
  cap        the literal
  threads    threads per workgroup of the launch
  per_trip   items the whole launch handles before its loop takes a second trip
  entry      the public entry that reaches the launcher
  test       the GPU test whose size goes past the cap, or None
  reason     why no test can go past the cap in seconds (exactly one of test / reason is given)

tests/test_cpu_launch_caps.py holds the table to the sources without a device: the literal must still stand in the launcher's body, and
the search must find no clamp that is not a row.  Whoever raises a cap sees that test fail with the name of the GPU test whose operands
must grow with it; without that, a second-trip test silently becomes a first-trip test.

The sizes of tests/test_gpu_launch_caps_exact.py are derived from the constants at the end of this file."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tensor4all-rs_amd", "csrc")
CAPS = (1024, 2048, 4096, 8192, 65535)
NEW = "test_gpu_launch_caps_exact.py::"


def row(file, launcher, capped, cap, threads, per_trip, entry, test=None, reason=None):
    return {"file": file, "launcher": launcher, "capped": capped, "cap": cap, "threads": threads, "per_trip": per_trip, "entry": entry,
            "test": test, "reason": reason}


RANK_1025 = "the clamped count is the rank of a factorisation: more than 1024 needs a rank-1025 rrLU or SVD, seconds per call"

TABLE = [
    # ---------------------------------------------------------------------------------------- kernels_tt.hip
    row("kernels_tt.hip", "permute_launch", "grid x", 4096, 256, 4096 * 256, "SimpleTensorTrain.reverse, LabelledTensor.permute",
        test=NEW + "test_permute_at_rank_3_and_at_the_largest_rank"),
    row("kernels_tt.hip", "col_scale_launch", "grid x", 1024, 256, 1024 * 256, "canonical.to_vidal (U * S of a bond)",
        reason="the rows of a bond matrix: more than 262 144 rows l * s on one core, whose SVD takes seconds"),
    row("kernels_tt.hip", "col_scale_launch", "grid y", 1024, 256, 1024, "canonical.to_vidal (U * S of a bond)", reason=RANK_1025),
    row("kernels_tt.hip", "core_reshape_launch", "grid x", 4096, 256, 4096 * 256, "SimpleTensorTrain.compress, TensorCI2.from_tensor_train",
        reason="a core above 1 048 576 elements is reshaped only in front of a factorisation of that core, which takes seconds"),
    row("kernels_tt.hip", "tt_norm2_step_launch", "grid x", 65535, 256, 65535 * 256, "SimpleTensorTrain.norm2",
        reason="r * r above 16 776 960 needs a bond of 4096 and 4096^2 * l^2 * s products per site"),
    row("kernels_tt.hip", "tt_env_left_launch", "grid x", 8192, 256, 8192, "SimpleTensorTrain.evaluate_many",
        test=NEW + "test_evaluate_many_past_8192_halves_and_2097152_points"),
    row("kernels_tt.hip", "tt_env_right_launch", "grid x", 8192, 256, 8192, "SimpleTensorTrain.evaluate_many",
        test=NEW + "test_evaluate_many_past_8192_halves_and_2097152_points"),
    row("kernels_tt.hip", "tt_env_dot_launch", "grid x", 8192, 256, 8192 * 256, "SimpleTensorTrain.evaluate_many",
        test=NEW + "test_evaluate_many_past_8192_halves_and_2097152_points"),
    # ---------------------------------------------------------------------------------------- tt.hip
    # (one clamp for four launches: tt_scale_kernel here, tt_site_sum_kernel in test_partial_sum_over_a_site_past_the_cap; tt_add2_kernel
    # runs on one-site trains, whose core of 1 x s x 1 holds at most 65535 elements: test_add_and_sub_of_one_site_trains_cannot_pass_the_cap)
    row("tt.hip", "blocks_for", "grid x", 4096, 256, 4096 * 256, "SimpleTensorTrain.scale / sub / partial_sum (add of one-site trains stays below)",
        test=NEW + "test_scale_of_a_last_core_past_the_cap"),
    # ---------------------------------------------------------------------------------------- kernels_dense.hip
    row("kernels_dense.hip", "gather_launch", "grid y", 1024, 256, 1024, "SimpleTensorTrain.add / sub (block copy)",
        test=NEW + "test_add_and_sub_block_copy"),
    row("kernels_dense.hip", "scatter_rows_launch", "grid y", 1024, 256, 1024, "matrix_luci_factors_from_matrix", reason=RANK_1025),
    row("kernels_dense.hip", "scatter_cols_launch", "grid y", 1024, 256, 1024, "matrix_luci_factors_from_matrix",
        test=NEW + "test_luci_factors_of_a_matrix_of_1030_columns"),
    row("kernels_dense.hip", "fill_launch", "grid x", 2048, 256, 2048 * 256, "SimpleTensorTrain.add / sub (block copy)",
        test=NEW + "test_add_and_sub_block_copy"),
    row("kernels_dense.hip", "set_identity_launch", "grid y", 1024, 256, 1024, "SimpleTensorTrain.partial_sum, matrix_luci_factors_from_matrix",
        test=NEW + "test_partial_sum_over_a_site_past_the_cap"),
    row("kernels_dense.hip", "tt_evaluate_launch", "grid x", 4096, 256, 4096, "SimpleTensorTrain.evaluate",
        test=NEW + "test_evaluate_9000_points_through_a_bond_of_300"),
    # ---------------------------------------------------------------------------------------- kernels_linalg.hip
    row("kernels_linalg.hip", "nonfinite_flag_launch", "grid x", 1024, 256, 1024 * 256, "svd_backend",
        reason="every entry runs nonfinite_absmax_launch over the same matrix first (Engine::svd), which refuses what this scan would "
               "find; behind it the scan sees the n x n factor of the QR, and 513 x 513 is a Jacobi iteration of seconds"),
    row("kernels_linalg.hip", "nonfinite_absmax_launch", "grid x", 1024, 256, 1024 * 256, "svd_backend, qr_backend",
        test=NEW + "test_svd_refuses_a_non_finite_entry_past_the_first_trip"),
    row("kernels_linalg.hip", "scale_pow2_launch", "grid x", 1024, 256, 1024 * 256, "svd_backend",
        test=NEW + "test_svd_and_qr_of_a_scaled_matrix_are_the_scaled_factors"),
    row("kernels_linalg.hip", "scale_pow2_dev_launch", "grid x", 1024, 256, 1024 * 256, "qr_backend",
        test=NEW + "test_svd_and_qr_of_a_scaled_matrix_are_the_scaled_factors"),
    row("kernels_linalg.hip", "jacobi_small_launch", "threads", 1024, 1024, 1024, "svd_backend",
        reason="a cap on the threads of one workgroup, not on a grid: Engine::svd_plain takes this kernel for n <= 16 only, 512 threads"),
    # ---------------------------------------------------------------------------------------- the dense tensor layer and the engine
    row("tensorops.hip", "diag_scale_launch", "grid x", 2048, 256, 2048 * 256, "LabelledTensor.factorize (SVD)",
        test=NEW + "test_factorize_svd_scales_540000_elements"),
    row("engine.hip", "tri_extract_launch", "grid y", 1024, 256, 1024, "matrix_luci_factors_from_matrix",
        test=NEW + "test_luci_factors_of_a_matrix_of_1030_columns"),
    # ---------------------------------------------------------------------------------------- multi-job element kernels
    row("kernels_swap.hip", "leg_reorder_launch", "grid x", 8192, 256, 8192 * 256, "LegTrain.reorder_legs",
        test=NEW + "test_reorder_legs_across_a_trip_boundary"),
    row("kernels_apply.hip", "apply_site_launch", "grid x", 8192, 256, 8192 * 256, "apply_linear_operator (naive, fused)",
        test=NEW + "test_apply_linear_operator_naive_fused_across_a_trip_boundary"),
    row("kernels_partial.hip", "mpo_partial_site_launch", "grid x", 8192, 256, 8192 * 256, "partial_contract (naive)",
        test=NEW + "test_partial_contract_naive_across_a_trip_boundary"),
    row("kernels_linsolve.hip", "builder_blocks", "grid x", 8192, 256, 8192 * 256, "linsolve._apply_env (half operators)",
        test=NEW + "test_linsolve_half_operators_past_the_cap"),
    row("kernels_mpo.hip", "mpo_site_contract_launch", "grid x", 8192, 256, 8192 * 256, "contract_naive",
        test="test_gpu_mpo_exact.py::test_naive_product_site_tensors"),
    row("kernels_pmpo.hip", "pmpo_launch_blocks", "grid x", 2048, 256, 2048 * 256, "partitioned.pair_products",
        test="test_gpu_pmpo_exact.py::test_pair_products_every_selector_at_every_position"),
    # ---------------------------------------------------------------------------------------- the TCI2 engine
    row("kernels_pi.hip", "pi_eval_launch", "grid y", 2048, 256, 2048, "TensorCI2.sweep2site",
        reason="more than 2048 columns of a Pi matrix: a bond above 1024 at d = 2, whose rrLU takes seconds per bond"),
    row("kernels_pi.hip", "absmax_launch", "grid x", 2048, 256, 2048 * 256, "TensorCI2.sweep2site, TensorCI2.from_tensor_train",
        reason="a Pi matrix or a core above 524 288 elements, in front of an rrLU of that matrix which takes seconds"),
    row("tci2.hip", "blocks_for", "grid x", 4096, 256, 4096 * 256, "TensorCI2.sweep2site",
        reason="a site tensor above 1 048 576 elements packed behind an rrLU of a Pi matrix of that size, seconds per bond"),
    row("kernels_chain.hip", "chain_pi_launch", "grid y", 2048, 256, 2048, "TensorCI2.optimize (bond chain)",
        reason="more than 2048 columns of a Pi matrix: a bond above 1024 at d = 2, whose rrLU takes seconds per bond"),
    row("kernels_chain.hip", "chain_pi_group_launch", "grid y", 2048, 256, 2048, "optimize_group (bond chain)",
        reason="more than 2048 columns of a Pi matrix: a bond above 1024 at d = 2, whose rrLU takes seconds per bond"),
    row("kernels_rrlu_global.hip", "rrlu_global_blocks", "grid x", 2048, 256, 2048 * 1024, "rrlu",
        test="test_gpu_rrlu_global.py::test_tall_and_large_shapes_match_oracle"),
    # ---------------------------------------------------------------------------------------- patching, aci, tree
    row("patching.hip", "make_selector_core", "grid x", 4096, 256, 4096 * 256, "adaptiveinterpolate",
        reason="bond * dim * bond above 1 048 576 needs a bond of 1024 at d = 2"),
    row("aci.hip", "matmul", "grid x", 4096, 256, 4096 * 256, "elementwise (frames of a local update)",
        reason="a frame product of more than 1 048 576 elements: bonds of several hundred on both sides, whose local update (an rrLU of "
               "the same matrix) takes seconds; the module has no hook that runs the product alone"),
    row("aci.hip", "AciProblem::local_update", "grid x", 8192, 256, 8192 * 256, "ElementwiseProblem.local_update",
        reason="more than 2 097 152 points of a local Pi matrix, which is then factorised by an rrLU of seconds"),
    row("aci.hip", "treeaci_local_update", "grid x", 8192, 256, 8192 * 256, "treeaci_local_update",
        reason="more than 2 097 152 points of a local Pi matrix, which is then factorised by an rrLU of seconds"),
    row("tree.hip", "TreeTci::chain_cores", "grid x", 1024, 256, 1024 * 256, "TreeTCI2.materialize",
        reason="a vertex tensor above 262 144 elements exists only behind tree sweeps with bonds of several hundred, seconds per edge"),
]

# hits of the search that clamp no launch: (file, function) -> what the line is
NOT_CLAMPS = {
    ("kernels_rrlu_xcd_common.hpp", "xcd2_tbl"): "the length of a table in the LDS (2048 or 1024 entries), chosen by the plan",
}

_NUM = "|".join(str(c) for c in CAPS)
_CLAMP = re.compile(r"(std::min\s*(<[^>]*>)?\s*\([^;]*[,(]\s*(%s)u?\s*\))|(if\s*\(\s*\w+\s*>\s*(%s)u?\s*\)\s*\w+\s*=\s*(%s)u?\s*;)|(<\s*(%s)u?\s*\?[^;:]*:\s*(%s)u?\b)|(\?\s*(%s)u?\s*:\s*(%s)u?\b)"
                    % ((_NUM,) * 7))
_DEF = re.compile(r"^[A-Za-z_].*\(")  # a definition starts in column 0 (kernels, launchers and methods alike)


def functions(text):
    """-> [(first line, last line, header)] of every function of a source: from a line that starts in column 0 and opens a parameter list
    to the next line that is a closing brace in column 0, or the line itself when it holds the whole body"""
    lines = text.split("\n")
    out, i = [], 0
    while i < len(lines):
        if not _DEF.match(lines[i]):
            i += 1
            continue
        j, opened = i, False
        while j < len(lines):
            code = lines[j].split("//")[0].rstrip()
            if not opened and "{" in code:
                opened = True
                if j == i and code.endswith("}"):
                    break  # the whole body on the line of the header
            elif not opened and code.endswith(";"):
                break  # a declaration, or a statement in column 0
            elif opened and lines[j].startswith("}"):
                break
            j += 1
        j = min(j, len(lines) - 1)
        if opened:
            out.append((i, j, lines[i]))
        i = j + 1
    return out


def header_names(header, launcher):
    """whether the first line of a function names `launcher` directly in front of its parameter list"""
    return re.search(r"(^|[\s*&:])%s\s*\(" % re.escape(launcher), header) is not None


def body_of(text, launcher):
    """the text of the function named `launcher`, or None"""
    lines = text.split("\n")
    for a, b, header in functions(text):
        if header_names(header, launcher):
            return "\n".join(lines[a:b + 1])
    return None


def count_literal(body, cap):
    return len(re.findall(r"(?<![\w.])%du?(?![\w.])" % cap, body))


def find_clamps(csrc=CSRC):
    """-> [(file, function header, line number, cap)] of every clamp in the sources"""
    hits = []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".hpp")):
            continue
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        lines = text.split("\n")
        fns = functions(text)
        for n, line in enumerate(lines):
            m = _CLAMP.search(line)
            if not m:
                continue
            cap = int(next(g for g in m.groups()[::-1] if g and g.rstrip("u").isdigit()).rstrip("u"))
            header = next((h for a, b, h in fns if a <= n <= b), "")
            hits.append((name, header, n + 1, cap))
    return hits


def rows_of(launcher, file=None):
    return [r for r in TABLE if r["launcher"] == launcher and (file is None or r["file"] == file)]


def per_trip(launcher, file=None, capped=None):
    rs = [r for r in rows_of(launcher, file) if capped is None or r["capped"] == capped]
    assert len(rs) == 1, (launcher, file, capped)
    return rs[0]["per_trip"]


# what the shapes of tests/test_gpu_launch_caps_exact.py are measured against
EVAL_POINTS = per_trip("tt_evaluate_launch")               # 4096 points, one workgroup each
ENV_ITEMS = per_trip("tt_env_left_launch")                 # 8192 environments per side
ENV_DOT_POINTS = per_trip("tt_env_dot_launch")             # 2 097 152 pairings
ELEMENTS_4096 = per_trip("blocks_for", "tt.hip")           # 1 048 576 elements: scale, add2, site sum
PERMUTE_ELEMENTS = per_trip("permute_launch")              # 1 048 576
COLUMNS_1024 = per_trip("gather_launch")                   # 1024 columns on gridDim.y
FILL_ELEMENTS = per_trip("fill_launch")                    # 524 288
SCAN_ELEMENTS = per_trip("nonfinite_absmax_launch")        # 262 144
DIAG_SCALE_ELEMENTS = per_trip("diag_scale_launch")        # 524 288
MULTI_JOB_OUTPUTS = per_trip("leg_reorder_launch")         # 2 097 152 outputs of the multi-job element kernels
BOND_STRIDE = 256                                          # `for (r = tid; r < R; r += 256)` of the chain kernels
