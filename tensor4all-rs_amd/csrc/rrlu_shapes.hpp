// rrlu_shapes.hpp — which instantiations of the register-resident rrLU kernel (kernels_rrlu_reg.hip and its _r2, _r3, _r4 builds) and
// of the one-workgroup rrLU kernel (kernels_rrlu_wg.hip, kernels_rrlu_wg_group.hip) exist, stated once.  The planners
// (rrlu_plan.hip, host code only) hand out no other shape; the launchers instantiate exactly these, in both tie orders, and throw
// on a plan outside the list.  tests/rrlu_plan_sweep.hip prints which shapes the planners select; tests/test_cpu_rrlu_plans.py
// holds that set against these lists, so an entry no matrix shape selects does not stay.
#pragma once
#include "kernels.hpp"

namespace t4a {

// ---- register-resident kernel: rrlu_reg_kernel<RPT, CPT, SINGLE, UNI, ROWMAJOR> ----
// X(RPT, CPT, SINGLE, UNI): rows / columns per thread; SINGLE: one workgroup (plan.W == 1); UNI: every wave lies inside one column
// group (plan.TR % 64 == 0).  One list per RPT: each is a translation unit of its own (kernels_rrlu_reg.hip and its _r2, _r3, _r4
// builds).  A multi-workgroup plan rounds TR to a multiple of 64 (always UNI), starts at three columns per thread and cannot hold
// RPT = 4 with CPT = 8 (more than 24 values per thread allow 256 threads, four row slots of a matrix beyond 64 x 64 need 448).
#define T4A_RRLU_REG_SHAPES_1(X)                                                                                                     \
    X(1, 1, true, false) X(1, 1, true, true) X(1, 2, true, false) X(1, 3, true, false) X(1, 3, true, true) X(1, 4, true, false)          \
    X(1, 5, true, false) X(1, 5, true, true) X(1, 6, true, false) X(1, 8, true, false)                                                  \
    X(1, 3, false, true) X(1, 4, false, true) X(1, 5, false, true) X(1, 6, false, true) X(1, 8, false, true)
#define T4A_RRLU_REG_SHAPES_2(X)                                                                                                     \
    X(2, 1, true, false) X(2, 1, true, true) X(2, 2, true, false) X(2, 3, true, false) X(2, 3, true, true) X(2, 4, true, false)          \
    X(2, 5, true, false) X(2, 5, true, true) X(2, 6, true, false) X(2, 8, true, false)                                                  \
    X(2, 3, false, true) X(2, 4, false, true) X(2, 5, false, true) X(2, 6, false, true) X(2, 8, false, true)
#define T4A_RRLU_REG_SHAPES_3(X)                                                                                                     \
    X(3, 1, true, false) X(3, 1, true, true) X(3, 2, true, false) X(3, 2, true, true) X(3, 3, true, false) X(3, 3, true, true)           \
    X(3, 4, true, false) X(3, 4, true, true)                                                                                           \
    X(3, 3, false, true) X(3, 4, false, true) X(3, 5, false, true) X(3, 6, false, true) X(3, 8, false, true)
#define T4A_RRLU_REG_SHAPES_4(X)                                                                                                     \
    X(4, 1, true, false) X(4, 1, true, true) X(4, 2, true, false) X(4, 2, true, true) X(4, 3, true, false) X(4, 3, true, true)           \
    X(4, 3, false, true) X(4, 4, false, true) X(4, 5, false, true) X(4, 6, false, true)
#define T4A_RRLU_REG_SHAPES(X) T4A_RRLU_REG_SHAPES_1(X) T4A_RRLU_REG_SHAPES_2(X) T4A_RRLU_REG_SHAPES_3(X) T4A_RRLU_REG_SHAPES_4(X)

struct RegShape {
    int rpt, cpt;
    bool single, uni;
};
#define T4A_X(R, C, S, U) {R, C, S, U},
constexpr RegShape kRegShapes[] = {T4A_RRLU_REG_SHAPES(T4A_X)};
#undef T4A_X
constexpr bool rrlu_reg_has_shape(int rpt, int cpt, bool single, bool uni)
{
    for (const RegShape& s : kRegShapes)
        if (s.rpt == rpt && s.cpt == cpt && s.single == single && s.uni == uni) return true;
    return false;
}
// smallest instantiated column count per thread >= c of the one-workgroup (single) or the multi-workgroup shapes, -1: none
constexpr int rrlu_reg_round_cpt(int c, bool single)
{
    int best = -1;
    for (const RegShape& s : kRegShapes)
        if (s.single == single && s.cpt >= c && (best < 0 || s.cpt < best)) best = s.cpt;
    return best;
}

// dynamic LDS of the register-resident kernel (internal linkage, as in the kernel's own file before: the planner's and every
// kernel unit's copy are inlined)
namespace {

struct RegSmem {
    double* urow;            // TC*CPT pivot-row entries of the owned columns
    double* lcol;            // M (single-workgroup mode only): raw pivot column
    double* red_sc;          // 16
    unsigned* red_pos;       // 16
    double* red_val;         // 16
    double* win_d;           // [0] value
    int* win_i;              // [0] winner wg  [1] position key  [2] abort flag
    unsigned short* posrow;  // M
    unsigned short* poscol;  // N
};

__host__ __device__ inline size_t align16(size_t v) { return (v + 15) / 16 * 16; }

__host__ __device__ inline size_t reg_smem_layout(int M, int N, int cols_per_wg, bool single, RegSmem* s, char* base)
{
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align16(off + bytes);
        return o;
    };
    const size_t o_urow = take((size_t)cols_per_wg * 8);
    const size_t o_lcol = take(single ? (size_t)M * 8 : 8);
    const size_t o_rsc = take(16 * 8);
    const size_t o_rpos = take(16 * 4);
    const size_t o_rval = take(16 * 8);
    const size_t o_wd = take(2 * 8);
    const size_t o_wi = take(4 * 4);
    const size_t o_pr = take((size_t)M * 2);
    const size_t o_pc = take((size_t)N * 2);
    if (s) {
        s->urow = (double*)(base + o_urow);
        s->lcol = (double*)(base + o_lcol);
        s->red_sc = (double*)(base + o_rsc);
        s->red_pos = (unsigned*)(base + o_rpos);
        s->red_val = (double*)(base + o_rval);
        s->win_d = (double*)(base + o_wd);
        s->win_i = (int*)(base + o_wi);
        s->posrow = (unsigned short*)(base + o_pr);
        s->poscol = (unsigned short*)(base + o_pc);
    }
    return off;
}

} // namespace

// ---- one-workgroup kernel: rrlu_wg_kernel<RPT, CPW, ROWMAJOR> and its group build ----
// X(RPT, CPW): rows per lane, columns per wave (a plan rounds the columns up to the next entry).  Beyond 16 values per lane
// (64 x 128, 128 x 64) the update — 2 readlanes + 3 RPT vector instructions per owned column, all on ONE compute unit — costs
// more than the single-XCD kernel's two L2 hand-offs (measured: tools/probe_wg.py), so the list ends there.
#define T4A_RRLU_WG_SHAPES(X) X(1, 8) X(1, 16) X(2, 8)

struct WgShape {
    int rpt, cpw;
};
#define T4A_X(R, C) {R, C},
constexpr WgShape kWgShapes[] = {T4A_RRLU_WG_SHAPES(T4A_X)};
#undef T4A_X
constexpr int WG_WAVES = 8; // waves per workgroup
// dynamic LDS of a shape (the kernel's layout is WgLds<RPT, CPW>, held against this by a static_assert beside it)
constexpr size_t wg_lds_bytes(int rpt, int cpw)
{
    const size_t MP = 64 * (size_t)rpt, NP = (size_t)WG_WAVES * cpw;
    return 2 * WG_WAVES * 16 + 2 * WG_WAVES * MP * 8 + 64 + MP * 8 + WG_WAVES * (2 * MP + 2 * NP) * 2;
}

} // namespace t4a
