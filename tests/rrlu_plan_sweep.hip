// rrlu_plan_sweep.hip — which kernel shapes the planners of the register-resident and the one-workgroup rrLU kernels hand out.
// Host code only: build it with the host-only planner file, no device code is needed
//   hipcc --cuda-host-only -O2 -std=c++17 tests/rrlu_plan_sweep.hip tensor4all-rs_amd/csrc/rrlu_plan.hip -o rrlu_plan_sweep
// It calls rrlu_reg_make_plan for every 1 <= M <= 4224, 1 <= N <= 2176 (past both planner limits: 4096 rows, 248 workgroups x 8
// columns) at 256, 64 and 16 compute units and rrlu_wg_make_plan for every 1 <= M <= 160, 1 <= N <= 640, and prints
//   reg-table RPT CPT SINGLE UNI            the instantiated shapes (rrlu_shapes.hpp)
//   reg CUS RPT CPT SINGLE UNI M N          every selected shape with its smallest witness (fewest entries, then fewest rows)
//   wg-table RPT CPW / wg RPT CPW M N       the same for the one-workgroup kernel
//   hash H                                  FNV-1a over every plan field in sweep order: equal hashes = equal decisions
// tests/test_cpu_rrlu_plans.py holds the selected sets against the tables.
#include <cstdint>
#include <cstdio>
#include <map>
#include <tuple>

#include "../tensor4all-rs_amd/csrc/rrlu_shapes.hpp"

using namespace t4a;

namespace {

uint64_t h = 1469598103934665603ull;
void mix(uint64_t v)
{
    for (int i = 0; i < 8; ++i) {
        h ^= (v >> (8 * i)) & 0xFFu;
        h *= 1099511628211ull;
    }
}

struct Witness {
    int M, N;
    bool better(int m, int n) const { return (long long)m * n < (long long)M * N || ((long long)m * n == (long long)M * N && m < M); }
};

} // namespace

int main()
{
    for (const RegShape& s : kRegShapes) std::printf("reg-table %d %d %d %d\n", s.rpt, s.cpt, (int)s.single, (int)s.uni);
    for (const int cus : {256, 64, 16}) {
        std::map<std::tuple<int, int, int, int>, Witness> seen;
        for (int M = 1; M <= 4224; ++M)
            for (int N = 1; N <= 2176; ++N) {
                RrluRegPlan p;
                const bool ok = rrlu_reg_make_plan(M, N, cus, &p);
                mix(ok);
                if (!ok) continue;
                for (const long long v : {(long long)p.W, (long long)p.T, (long long)p.TR, (long long)p.TC, (long long)p.RPT, (long long)p.CPT,
                                          (long long)p.lds_bytes, (long long)rrlu_reg_keys_bytes(p), (long long)rrlu_reg_cols_bytes(p, M)})
                    mix((uint64_t)v);
                const auto key = std::make_tuple(p.RPT, p.CPT, (int)(p.W == 1), (int)(p.TR % 64 == 0));
                const auto it = seen.find(key);
                if (it == seen.end()) seen[key] = Witness{M, N};
                else if (it->second.better(M, N)) it->second = Witness{M, N};
            }
        for (const auto& kv : seen)
            std::printf("reg %d %d %d %d %d %d %d\n", cus, std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), std::get<3>(kv.first),
                        kv.second.M, kv.second.N);
    }
    for (const WgShape& s : kWgShapes) std::printf("wg-table %d %d\n", s.rpt, s.cpw);
    std::map<std::pair<int, int>, Witness> seen;
    for (int M = 1; M <= 160; ++M)
        for (int N = 1; N <= 640; ++N) {
            RrluXcdPlan p;
            const bool ok = rrlu_wg_make_plan(M, N, &p, 0);
            mix(ok);
            if (!ok) continue;
            for (const long long v : {(long long)p.W, (long long)p.RPT, (long long)p.CPT, (long long)p.grid, (long long)p.lds_bytes, (long long)p.wg})
                mix((uint64_t)v);
            const auto key = std::make_pair(p.RPT, p.CPT);
            const auto it = seen.find(key);
            if (it == seen.end()) seen[key] = Witness{M, N};
            else if (it->second.better(M, N)) it->second = Witness{M, N};
        }
    for (const auto& kv : seen) std::printf("wg %d %d %d %d\n", kv.first.first, kv.first.second, kv.second.M, kv.second.N);
    std::printf("hash %016llx\n", (unsigned long long)h);
    return 0;
}
