// rrlu_plan.hip — launch plans of the chip-wide register-resident rrLU kernel (kernels_rrlu_reg.hip) and of the one-workgroup
// kernel (kernels_rrlu_wg.hip): which instantiation of rrlu_shapes.hpp takes a given shape, and the size of its exchange buffers.
// Host code only (the plans of the single-XCD family are in rrlu_xcd_plan.hip).
#include "rrlu_shapes.hpp"

#include <algorithm>
#include <cstdlib>

namespace t4a {

namespace {

int round_up(int v, int m) { return (v + m - 1) / m * m; }

} // namespace

bool rrlu_reg_make_plan(int M, int N, int num_cus, RrluRegPlan* out)
{
    RrluRegPlan plan;
    // (the key-table poller reads 4 keys per lane and the engine reserves 256 slots: never plan more workgroups than that)
    const int maxw = std::min(num_cus > 16 ? num_cus - 8 : num_cus, 256);
    const long long elems = (long long)M * N;
    bool found = false;
    if (elems <= 64 * 64) {
        // one workgroup: TR x TC thread grid with <= 4 x 8 elements per thread; minimise the per-thread work,
        // then the thread count
        int best_cost = 1 << 30;
        for (int T = 64; T <= 512; T *= 2) {
            for (int TR = 16; TR <= T; TR *= 2) {
                const int TC = T / TR;
                const int RPT = (M + TR - 1) / TR;
                const int CPT = rrlu_reg_round_cpt((N + TC - 1) / TC, true);
                if (CPT < 0 || !rrlu_reg_has_shape(RPT, CPT, true, TR % 64 == 0)) continue;
                if (T > ((RPT * CPT > 24) ? 256 : 512)) continue;
                const int cost = RPT * CPT * 64 + T / 64;
                if (cost < best_cost) {
                    best_cost = cost;
                    plan.W = 1;
                    plan.T = T;
                    plan.TR = TR;
                    plan.TC = TC;
                    plan.RPT = RPT;
                    plan.CPT = CPT;
                    found = true;
                }
            }
        }
    }
    if (!found) {
        int RPT = (M + 511) / 512; // two waves per SIMD hide the f64 issue latency (measured: T=512 beats 256)
        if (RPT > 4) RPT = 4;
        int TR = round_up((M + RPT - 1) / RPT, 64);
        int TC = 1;
        if (TR < 256) TC = 256 / TR;
        if (TR > 1024) return false; // beyond the register budget: LDS kernel
        // more, thinner workgroups win once the key table is shared (measured: 3 columns per thread and 230 workgroups
        // beat 4 / 172 by 3.5 % at 685 x 688); the wider shapes follow when that would need more workgroups than CUs
        int CPT = 0, W = 0;
        for (int c = rrlu_reg_round_cpt(1, false); c > 0 && (CPT == 0 || W > maxw); c = rrlu_reg_round_cpt(c + 1, false)) {
            CPT = c; // 3 -> 4 -> 5 -> 6 -> 8 columns per thread
            W = (N + TC * CPT - 1) / (TC * CPT);
        }
        if (W < 1) W = 1;
        if (W > maxw || (long long)W * TC * CPT < N) return false;
        if (TR * TC > ((RPT * CPT > 24) ? 256 : 512)) return false;
        if (!rrlu_reg_has_shape(RPT, CPT, W == 1, true)) return false;
        plan.W = W;
        plan.T = TR * TC;
        plan.TR = TR;
        plan.TC = TC;
        plan.RPT = RPT;
        plan.CPT = CPT;
    }
    plan.lds_bytes = reg_smem_layout(M, N, plan.TC * plan.CPT, plan.W == 1, nullptr, nullptr);
    if (plan.lds_bytes > 160 * 1024) return false;
    if (plan.W > 1 && plan.lds_bytes < 84 * 1024) plan.lds_bytes = 84 * 1024; // one workgroup per CU
    *out = plan;
    return true;
}

size_t rrlu_reg_keys_bytes(const RrluRegPlan& plan)
{
    return (size_t)2 * plan.W * 2 * sizeof(unsigned long long);
}
size_t rrlu_reg_cols_bytes(const RrluRegPlan& plan, int M)
{
    const size_t slots = (size_t)(plan.W > RRLU_MAX_COPIES ? plan.W : RRLU_MAX_COPIES); // one per workgroup: every workgroup may publish its candidate column with its key
    return (size_t)2 * slots * (size_t)M * 2 * sizeof(unsigned long long);
}

// One-workgroup plan for an M x N matrix (upper bounds in a bond chain), or false when it does not fit.  spec_blocks: workgroups
// beside the factorising one that evaluate the next bond's candidate matrix (bond chain, solo launch).
bool rrlu_wg_make_plan(int M, int N, RrluXcdPlan* out, int spec_blocks)
{
    static const bool off = std::getenv("T4A_NO_WG") != nullptr;
    if (off || M < 1 || N < 1) return false;
    const int rpt = (M + 63) / 64;
    const int need = (N + WG_WAVES - 1) / WG_WAVES;
    int cpw = -1;
    for (const WgShape& s : kWgShapes)
        if (s.rpt == rpt && need <= s.cpw && (cpw < 0 || s.cpw < cpw)) cpw = s.cpw;
    if (cpw < 0) return false;
    RrluXcdPlan plan;
    plan.W = 1;
    plan.RPT = rpt;
    plan.CPT = cpw;
    plan.grid = 1 + (spec_blocks > 0 ? spec_blocks : 0);
    plan.lds_bytes = wg_lds_bytes(rpt, cpw);
    plan.wg = 1;
    *out = plan;
    return true;
}

} // namespace t4a
