// pmpo.hip — partitioned MPOs on the device (see pmpo.hpp).  Projector algebra and the task list are host work; the floating-point work
// runs in gfx950 kernels: the mask launch, the fused pair-product launch and the direct sum of to_mpo (kernels_pmpo.hip), TensorTrain::add, the
// compress stage and the zip-up of mpo.hip.
#include "pmpo.hpp"
#include "patching.hpp"

#include <chrono>
#include <climits>
#include <cmath>
#include <string>

namespace t4a {

// ------------------------------------------------------------------------------------------------ projector.rs
LegProjector projector_from_triples(const size_t* triples, size_t count)
{
    LegProjector p;
    if (count && !triples) throw Error(T4A_GPU_NULL_POINTER, "projector entries are null");
    for (size_t i = 0; i < count; ++i) {
        const size_t site = triples[3 * i], leg = triples[3 * i + 1], value = triples[3 * i + 2];
        if (leg > 1)
            throw Error(T4A_GPU_INVALID_ARGUMENT,
                        "projector leg " + std::to_string(leg) + " at site " + std::to_string(site) + " is neither 0 (s1) nor 1 (s2)");
        p[{site, leg}] = value; // from_pairs: the last pair of a key replaces the earlier one
    }
    return p;
}

void projector_validate(const LegProjector& p, const SiteDims& sd)
{
    for (const auto& kv : p) {
        const size_t site = kv.first.first, leg = kv.first.second;
        if (site >= sd.size())
            throw Error(T4A_GPU_INVALID_ARGUMENT, "projector index (site " + std::to_string(site) + ", leg " + std::to_string(leg) +
                                                      ") is absent from the chain of " + std::to_string(sd.size()) + " sites");
        const size_t dim = sd[site][leg];
        if (kv.second >= dim)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "projector coordinate " + std::to_string(kv.second) + " is out of range for index (site " +
                                                      std::to_string(site) + ", leg " + std::to_string(leg) + ") with dimension " +
                                                      std::to_string(dim));
    }
}

bool projector_intersection(const LegProjector& a, const LegProjector& b, LegProjector& out)
{
    out = a;
    for (const auto& kv : b) {
        auto it = out.find(kv.first);
        if (it == out.end()) out.insert(kv);
        else if (it->second != kv.second) return false;
    }
    return true;
}

bool projector_compatible(const LegProjector& a, const LegProjector& b)
{
    LegProjector tmp;
    return projector_intersection(a, b, tmp);
}

LegProjector projector_common_restriction(const LegProjector& a, const LegProjector& b)
{
    LegProjector out;
    for (const auto& kv : a) {
        auto it = b.find(kv.first);
        if (it != b.end() && it->second == kv.second) out.insert(kv);
    }
    return out;
}

bool projector_is_subset_of(const LegProjector& a, const LegProjector& b)
{
    for (const auto& kv : b) {
        auto it = a.find(kv.first);
        if (it == a.end() || it->second != kv.second) return false;
    }
    return a.size() >= b.size();
}

bool projectors_disjoint(const std::vector<LegProjector>& ps)
{
    for (size_t i = 0; i < ps.size(); ++i)
        for (size_t j = i + 1; j < ps.size(); ++j)
            if (projector_compatible(ps[i], ps[j])) return false;
    return true;
}

LegProjector projector_filter(const LegProjector& p, const std::vector<std::pair<size_t, size_t>>& keys)
{
    LegProjector out;
    for (const auto& k : keys) {
        auto it = p.find(k);
        if (it != p.end()) out.insert(*it);
    }
    return out;
}

int projector_compare(const LegProjector& a, const LegProjector& b)
{
    auto x = a.begin(), y = b.begin();
    for (; x != a.end() && y != b.end(); ++x, ++y) {
        if (x->first != y->first) return x->first < y->first ? -1 : 1;
        if (x->second != y->second) return x->second < y->second ? -1 : 1;
    }
    if (x == a.end() && y == b.end()) return 0;
    return x == a.end() ? -1 : 1;
}

// ------------------------------------------------------------------------------------------------ contraction_tasks
PmpoPlan pmpo_contract_plan(const std::vector<LegProjector>& pa, const std::vector<LegProjector>& pb)
{
    PmpoPlan plan;
    for (size_t i = 0; i < pa.size(); ++i)
        for (size_t j = 0; j < pb.size(); ++j) {
            bool ok = true;
            for (const auto& kv : pa[i]) {
                if (kv.first.second != 1) continue;
                auto it = pb[j].find({kv.first.first, 0});
                if (it != pb[j].end() && it->second != kv.second) {
                    ok = false;
                    break;
                }
            }
            if (!ok) continue;
            LegProjector r;
            for (const auto& kv : pa[i])
                if (kv.first.second == 0) r.insert(kv);
            for (const auto& kv : pb[j])
                if (kv.first.second == 1) r.insert(kv);
            size_t k = 0;
            while (k < plan.results.size() && plan.results[k] != r) ++k;
            if (k == plan.results.size()) plan.results.push_back(r);
            plan.tasks.push_back({i, j, k});
        }
    return plan;
}

namespace {

void check_site_count(size_t a, size_t b, size_t c, size_t d, const std::string& what)
{
    const unsigned long long lim = INT_MAX;
    unsigned long long n = 1;
    for (size_t x : {a, b, c, d}) {
        if (x > lim || n * x > lim) throw Error(T4A_GPU_INVALID_ARGUMENT, what + " holds more than INT_MAX elements");
        n *= x;
    }
}

long long selector(const LegProjector& p, size_t site, size_t leg)
{
    auto it = p.find({site, leg});
    return it == p.end() ? -1 : (long long)it->second;
}

std::vector<LegProjector> projectors_of(const PartitionedMpo& m)
{
    std::vector<LegProjector> v;
    for (const auto& p : m.patches) v.push_back(p.proj);
    return v;
}

// a rank rule that keeps every singular value (tolerance 0, no cap) cuts nothing: the sweep would only change the gauge
bool truncates(const MpoContractionOptions& o) { return o.tolerance != 0.0 || o.max_bond_dim != 0; }

// project every listed chain onto its projector: one job per site that carries a projected leg, ONE launch for all of them
void mask_chains(Engine& eng, const std::vector<std::vector<DevCore>*>& chains, const std::vector<const LegProjector*>& projs,
                 const SiteDims& sd)
{
    std::vector<PmpoMaskJob> jobs;
    unsigned long long off = 0;
    for (size_t c = 0; c < chains.size(); ++c)
        for (size_t i = 0; i < chains[c]->size(); ++i) {
            const long long m1 = selector(*projs[c], i, 0), m2 = selector(*projs[c], i, 1);
            if (m1 < 0 && m2 < 0) continue;
            DevCore& x = (*chains[c])[i];
            check_site_count(x.l, sd[i][0], sd[i][1], x.r, "project: patch " + std::to_string(c) + ", site " + std::to_string(i));
            PmpoMaskJob j{};
            j.X = x.buf.get();
            j.off = off;
            j.l = (int)x.l, j.s1 = (int)sd[i][0], j.s2 = (int)sd[i][1], j.r = (int)x.r;
            j.m1 = (int)m1, j.m2 = (int)m2;
            jobs.push_back(j);
            off += x.size();
        }
    if (jobs.empty()) return;
    if (jobs.size() > (size_t)INT_MAX) throw Error(T4A_GPU_INVALID_ARGUMENT, "project: more than INT_MAX sites to mask");
    DevBuf<PmpoMaskJob> d_jobs;
    d_jobs.reserve(jobs.size());
    T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(PmpoMaskJob), hipMemcpyHostToDevice, eng.stream()));
    pmpo_mask_launch(d_jobs.get(), (int)jobs.size(), off, eng.stream());
    T4A_HIP(hipGetLastError());
    eng.sync(); // `jobs` is pageable host memory, d_jobs goes out of scope
}

// the job of one site of one task; the output core is made here
PmpoPairJob pair_job(const PmpoPatch& pa, const PmpoPatch& pb, const SiteDims& sda, const SiteDims& sdb, size_t task, size_t i, DevCore& out,
                     unsigned long long off)
{
    const DevCore& x = pa.mpo->tt.cores[i];
    const DevCore& y = pb.mpo->tt.cores[i];
    const size_t s1 = sda[i][0], k = sda[i][1], t = sdb[i][1];
    check_site_count(x.l * y.l, s1, t, x.r * y.r, "contract: task " + std::to_string(task) + ", site " + std::to_string(i));
    out = DevCore::make(x.l * y.l, s1 * t, x.r * y.r);
    PmpoPairJob j{};
    j.A = x.buf.get();
    j.B = y.buf.get();
    j.C = out.buf.get();
    j.off = off;
    j.la = (int)x.l, j.s1 = (int)s1, j.k = (int)k, j.ra = (int)x.r, j.lb = (int)y.l, j.t = (int)t, j.rb = (int)y.r;
    // the contracted leg: one value where either operand projects it (they agree where both do), otherwise the full range
    long long kv = selector(pa.proj, i, 1);
    if (kv < 0) kv = selector(pb.proj, i, 0);
    j.k0 = kv < 0 ? 0 : (int)kv;
    j.k1 = kv < 0 ? (int)k : (int)kv + 1;
    j.sm = (int)selector(pa.proj, i, 0);
    j.tm = (int)selector(pb.proj, i, 1);
    return j;
}

void launch_pairs(Engine& eng, const std::vector<PmpoPairJob>& jobs, unsigned long long total)
{
    if (jobs.empty()) return;
    if (jobs.size() > (size_t)INT_MAX) throw Error(T4A_GPU_INVALID_ARGUMENT, "contract: more than INT_MAX site products");
    DevBuf<PmpoPairJob> d_jobs;
    d_jobs.reserve(jobs.size());
    T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(PmpoPairJob), hipMemcpyHostToDevice, eng.stream()));
    pmpo_pair_contract_launch(d_jobs.get(), (int)jobs.size(), total, eng.stream());
    T4A_HIP(hipGetLastError());
    eng.sync(); // `jobs` is pageable host memory, d_jobs goes out of scope
}

// the shape checks of mpo_contract, with its messages
void check_operands(const PartitionedMpo& a, const PartitionedMpo& b)
{
    if (a.sd.size() != b.sd.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT,
                    "MPO length mismatch: expected " + std::to_string(a.sd.size()) + ", got " + std::to_string(b.sd.size()));
    for (size_t i = 0; i < a.sd.size(); ++i)
        if (a.sd[i][1] != b.sd[i][0])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Shared shape mismatch at site " + std::to_string(i) + ": MPO A has site_dim_2=" +
                                                      std::to_string(a.sd[i][1]) + ", MPO B has site_dim_1=" + std::to_string(b.sd[i][0]));
}

void sync_all(PartitionedMpo& m)
{
    for (auto& p : m.patches) p.mpo->tt.eng.sync();
}

// x + y by direct sum, truncated where the rank rule can cut (add_reindexed_like_self + truncate, partitioned_tt.rs:317-332)
std::unique_ptr<Mpo> add_truncate(Mpo& x, Mpo& y, bool truncate, const MpoContractionOptions& opt)
{
    std::unique_ptr<TensorTrain> s = x.tt.add(y.tt, false);
    std::vector<DevCore> cores = std::move(s->cores);
    if (truncate) mpo_compress_cores(x.tt.eng, cores, opt);
    return std::make_unique<Mpo>(std::move(cores), x.sd);
}

} // namespace

void pmpo_mask_chains(Engine& eng, const std::vector<std::vector<DevCore>*>& chains, const std::vector<const LegProjector*>& projs,
                      const SiteDims& sd)
{
    mask_chains(eng, chains, projs, sd);
}

// ------------------------------------------------------------------------------------------------ the handle
void PartitionedMpo::validate(const SiteDims& sd, const std::vector<SiteDims>& patch_dims, const std::vector<LegProjector>& projectors)
{
    if (patch_dims.size() != projectors.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "partitioned MPO: " + std::to_string(patch_dims.size()) + " patches but " +
                                                  std::to_string(projectors.size()) + " projectors");
    for (size_t k = 0; k < patch_dims.size(); ++k) {
        if (patch_dims[k].size() != sd.size())
            throw Error(T4A_GPU_INVALID_ARGUMENT, "partitioned MPO: patch " + std::to_string(k) + " has " + std::to_string(patch_dims[k].size()) +
                                                      " sites, the chain has " + std::to_string(sd.size()));
        for (size_t i = 0; i < sd.size(); ++i)
            if (patch_dims[k][i] != sd[i])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "partitioned MPO: patch " + std::to_string(k) + " has site dims (" +
                                                          std::to_string(patch_dims[k][i][0]) + ", " + std::to_string(patch_dims[k][i][1]) +
                                                          ") at site " + std::to_string(i) + ", the chain has (" + std::to_string(sd[i][0]) +
                                                          ", " + std::to_string(sd[i][1]) + ")");
    }
    for (const auto& p : projectors) projector_validate(p, sd);
    for (size_t i = 0; i < projectors.size(); ++i)
        for (size_t j = i + 1; j < projectors.size(); ++j)
            if (projector_compatible(projectors[i], projectors[j]))
                throw Error(T4A_GPU_INVALID_ARGUMENT,
                            "Projectors overlap: patches " + std::to_string(i) + " and " + std::to_string(j) + " are not disjoint");
}

std::unique_ptr<PartitionedMpo> PartitionedMpo::from_patches(const std::vector<Mpo*>& ms, const std::vector<LegProjector>& projectors,
                                                             const SiteDims* site_dims)
{
    SiteDims sd;
    if (site_dims) sd = *site_dims;
    else if (!ms.empty()) sd = ms[0]->sd;
    std::vector<SiteDims> pd;
    for (Mpo* m : ms) pd.push_back(m->sd);
    validate(sd, pd, projectors);
    auto out = std::make_unique<PartitionedMpo>(sd);
    for (size_t k = 0; k < ms.size(); ++k)
        out->patches.push_back({projectors[k], std::make_unique<Mpo>(ms[k]->tt.cores, ms[k]->tt.eng.stream(), sd)});
    return out;
}

std::unique_ptr<PartitionedMpo> PartitionedMpo::from_ptt(PartitionedTT& src, const size_t* site_dims)
{
    const size_t n = src.dims.size();
    SiteDims fused(n), sd(n);
    for (size_t i = 0; i < n; ++i) {
        fused[i] = {src.dims[i], 1};
        sd[i] = site_dims ? std::array<size_t, 2>{site_dims[2 * i], site_dims[2 * i + 1]} : fused[i];
        if (sd[i][0] == 0 || sd[i][0] * sd[i][1] != src.dims[i])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "relabel_site_dims: site " + std::to_string(i) + " has " + std::to_string(src.dims[i]) +
                                                      " fused indices, not " + std::to_string(sd[i][0]) + " * " + std::to_string(sd[i][1]));
    }
    auto r = std::make_unique<PartitionedMpo>(sd);
    for (const SubDomain& p : src.patches) {
        LegProjector proj;
        for (const auto& kv : p.projector) {
            proj[{kv.first, 0}] = kv.second % sd[kv.first][0];
            proj[{kv.first, 1}] = kv.second / sd[kv.first][0];
        }
        auto m = std::make_unique<Mpo>(p.cores, src.eng.stream(), fused);
        m->relabel_site_dims(sd);
        r->patches.push_back({proj, std::move(m)});
    }
    return r;
}

double PartitionedMpo::norm()
{
    double sum_sq = 0.0;
    for (auto& p : patches) sum_sq = sum_sq + p.mpo->tt.norm2(); // the train's norm2 is the squared Frobenius norm
    return std::sqrt(sum_sq);
}

std::vector<double> PartitionedMpo::evaluate(const uint32_t* idx, size_t n_pts)
{
    const size_t n = sd.size();
    if (n == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "MPO is empty");
    for (size_t p = 0; p < n_pts; ++p)
        for (size_t s = 0; s < n; ++s) {
            const uint32_t i = idx[2 * n * p + 2 * s], j = idx[2 * n * p + 2 * s + 1];
            if (i >= sd[s][0] || j >= sd[s][1])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "Index out of bounds: index " + std::to_string(std::max(i, j)) + " at site " +
                                                          std::to_string(s) + " (max: " + std::to_string(std::max(sd[s][0], sd[s][1])) + ")");
        }
    std::vector<double> out(n_pts, 0.0);
    for (auto& p : patches) {
        const std::vector<double> part = p.mpo->evaluate(idx, n_pts);
        for (size_t q = 0; q < n_pts; ++q) out[q] = out[q] + part[q]; // patch order, like PartitionedTT::evaluate
    }
    return out;
}

std::unique_ptr<PartitionedMpo> PartitionedMpo::project(const LegProjector& p)
{
    projector_validate(p, sd);
    auto out = std::make_unique<PartitionedMpo>(sd);
    for (auto& q : patches) {
        LegProjector merged;
        if (!projector_intersection(q.proj, p, merged)) continue; // no overlap: the patch is dropped (subdomain_tt.rs:185-188)
        out->patches.push_back({merged, std::make_unique<Mpo>(q.mpo->tt.cores, q.mpo->tt.eng.stream(), sd)});
    }
    if (out->patches.empty()) return out;
    std::vector<std::vector<DevCore>*> chains;
    std::vector<const LegProjector*> projs;
    for (auto& q : out->patches) {
        chains.push_back(&q.mpo->tt.cores);
        projs.push_back(&q.proj);
    }
    mask_chains(out->patches[0].mpo->tt.eng, chains, projs, sd);
    return out;
}

std::unique_ptr<PartitionedMpo> PartitionedMpo::add(PartitionedMpo& other, const MpoContractionOptions& opt)
{
    if (sd != other.sd) throw Error(T4A_GPU_INVALID_ARGUMENT, "add: the partitioned MPOs have different lengths or site dims");
    std::vector<LegProjector> uni = projectors_of(*this);
    for (const auto& q : other.patches) {
        bool have = false;
        for (const auto& u : uni) have = have || u == q.proj;
        if (!have) uni.push_back(q.proj);
    }
    if (!projectors_disjoint(uni))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Incompatible projectors: Projectors must be pairwise disjoint for patch-wise addition");
    auto out = std::make_unique<PartitionedMpo>(sd);
    for (auto& q : patches) {
        PmpoPatch* match = nullptr;
        for (auto& o : other.patches)
            if (o.proj == q.proj) match = &o;
        if (match) out->patches.push_back({q.proj, add_truncate(*q.mpo, *match->mpo, truncates(opt), opt)});
        else out->patches.push_back({q.proj, std::make_unique<Mpo>(q.mpo->tt.cores, q.mpo->tt.eng.stream(), sd)});
    }
    for (auto& o : other.patches) {
        bool have = false;
        for (const auto& q : patches) have = have || q.proj == o.proj;
        if (!have) out->patches.push_back({o.proj, std::make_unique<Mpo>(o.mpo->tt.cores, o.mpo->tt.eng.stream(), sd)});
    }
    return out;
}

std::unique_ptr<Mpo> PartitionedMpo::to_mpo(int route)
{
    if (patches.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "Partitioned tensor train is empty");
    if (route < 0 || route > 2) throw Error(T4A_GPU_INVALID_ARGUMENT, "to_mpo: route 0 (the rule), 1 (pairwise adds) or 2 (one launch)");
    std::vector<size_t> order(patches.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(),
                     [&](size_t x, size_t y) { return projector_compare(patches[x].proj, patches[y].proj) < 0; });
    const size_t n = sd.size(), G = order.size();
    // one site: the direct sum is the plain sum of the values, which the train addition forms; one patch: a copy
    const bool ragged = route != 1; // the rule: measured faster at every size tried
    if (!ragged || n < 2 || G < 2) {
        Mpo& first = *patches[order[0]].mpo;
        auto acc = std::make_unique<Mpo>(first.tt.cores, first.tt.eng.stream(), sd);
        for (size_t k = 1; k < G; ++k) acc = add_truncate(*acc, *patches[order[k]].mpo, false, MpoContractionOptions{});
        return acc;
    }
    // every site of the direct sum in one launch (kernels_pmpo.hip: pmpo_direct_sum_kernel)
    sync_all(*this);
    Engine& eng = patches[order[0]].mpo->tt.eng;
    std::vector<DevCore> out(n);
    std::vector<PmpoSumJob> jobs(n);
    std::vector<const double*> src(n * G);
    std::vector<int> offs(2 * n * (G + 1));
    DevBuf<const double*> d_src;
    DevBuf<int> d_offs;
    DevBuf<PmpoSumJob> d_jobs;
    d_src.reserve(n * G);
    d_offs.reserve(2 * n * (G + 1));
    d_jobs.reserve(n);
    unsigned long long off = 0;
    for (size_t i = 0; i < n; ++i) {
        int* row0 = offs.data() + 2 * i * (G + 1);
        int* col0 = row0 + (G + 1);
        size_t L = 0, R = 0;
        for (size_t g = 0; g < G; ++g) {
            const DevCore& c = patches[order[g]].mpo->tt.cores[i];
            src[i * G + g] = c.buf.get();
            row0[g] = (int)L;
            col0[g] = (int)R;
            L += c.l;
            R += c.r;
        }
        if (i == 0) L = 1;
        if (i == n - 1) R = 1;
        row0[G] = (int)L;
        col0[G] = (int)R;
        const size_t S = sd[i][0] * sd[i][1];
        check_site_count(L, S, 1, R, "to_mpo: site " + std::to_string(i));
        if (L > 65535 || R > 65535) throw Error(T4A_GPU_INVALID_ARGUMENT, "to_mpo: site " + std::to_string(i) + ": bonds above 65535 are not supported");
        out[i] = DevCore::make(L, S, R);
        PmpoSumJob& j = jobs[i];
        j = PmpoSumJob{};
        j.dst = out[i].buf.get();
        j.src = d_src.get() + i * G;
        j.row0 = d_offs.get() + 2 * i * (G + 1);
        j.col0 = j.row0 + (G + 1);
        j.off = off;
        j.L = (int)L, j.S = (int)S, j.R = (int)R, j.G = (int)G, j.first = i == 0, j.last = i == n - 1;
        off += out[i].size();
    }
    const hipStream_t st = eng.stream();
    T4A_HIP(hipMemcpyAsync(d_src.get(), src.data(), src.size() * sizeof(const double*), hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(d_offs.get(), offs.data(), offs.size() * sizeof(int), hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), jobs.size() * sizeof(PmpoSumJob), hipMemcpyHostToDevice, st));
    pmpo_direct_sum_launch(d_jobs.get(), (int)n, off, st);
    T4A_HIP(hipGetLastError());
    eng.sync(); // the host arrays are pageable memory, the device arrays go out of scope
    return std::make_unique<Mpo>(std::move(out), sd);
}

std::unique_ptr<PartitionedMpo> PartitionedMpo::contract(PartitionedMpo& other, MpoAlgorithm alg, bool compress, const MpoContractionOptions& opt,
                                                         CompressRoute compress_route)
{
    check_operands(*this, other);
    if (alg == MpoAlgorithm::ZipUp && compress_route == CompressRoute::Batched)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "contract: the batched compress route needs the naive algorithm (the SVDs of zip-up interleave with "
                                              "its products)");
    if (alg == MpoAlgorithm::Fit) // contract_fit.rs:65-96
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "Unsupported operation: simplett variational MPO fitting is not implemented; use contract_naive or "
                                             "contract_zipup instead");
    const size_t n = sd.size();
    SiteDims rsd(n);
    for (size_t i = 0; i < n; ++i) rsd[i] = {sd[i][0], other.sd[i][1]};
    auto out = std::make_unique<PartitionedMpo>(rsd);
    const PmpoPlan plan = pmpo_contract_plan(projectors_of(*this), projectors_of(other));
    // result.insert (partitioned_tt.rs:196-210, :334) refuses a result whose projector overlaps another one without being equal to it
    for (size_t i = 0; i < plan.results.size(); ++i)
        for (size_t j = i + 1; j < plan.results.size(); ++j)
            if (projector_compatible(plan.results[i], plan.results[j]))
                throw Error(T4A_GPU_INVALID_ARGUMENT,
                            "Projectors overlap: results " + std::to_string(i) + " and " + std::to_string(j) + " of the contraction are not disjoint");
    if (plan.tasks.empty() || n == 0) return out;
    const size_t nt = plan.tasks.size();
    Engine& eng = patches[plan.tasks[0].a].mpo->tt.eng;
    sync_all(*this);
    sync_all(other);
    std::vector<std::unique_ptr<Mpo>> products(nt);
    if (alg == MpoAlgorithm::ZipUp) {
        // the products of zip-up interleave with its SVDs: mask copies of the operands (apply_projection) in one launch, then the
        // existing zip-up per task
        std::unique_ptr<PartitionedMpo> ma = std::make_unique<PartitionedMpo>(sd), mb = std::make_unique<PartitionedMpo>(other.sd);
        std::vector<std::vector<DevCore>*> chains;
        std::vector<const LegProjector*> projs;
        for (auto& q : patches) ma->patches.push_back({q.proj, std::make_unique<Mpo>(q.mpo->tt.cores, nullptr, sd)});
        for (auto& q : other.patches) mb->patches.push_back({q.proj, std::make_unique<Mpo>(q.mpo->tt.cores, nullptr, other.sd)});
        // one launch needs one site-dims table: A's patches and B's patches go in two launches only when their site dims differ
        for (auto& q : ma->patches) chains.push_back(&q.mpo->tt.cores), projs.push_back(&q.proj);
        if (sd == other.sd) {
            for (auto& q : mb->patches) chains.push_back(&q.mpo->tt.cores), projs.push_back(&q.proj);
            mask_chains(eng, chains, projs, sd);
        } else {
            mask_chains(eng, chains, projs, sd);
            chains.clear();
            projs.clear();
            for (auto& q : mb->patches) chains.push_back(&q.mpo->tt.cores), projs.push_back(&q.proj);
            mask_chains(eng, chains, projs, other.sd);
        }
        for (size_t t = 0; t < nt; ++t)
            products[t] = mpo_contract(*ma->patches[plan.tasks[t].a].mpo, *mb->patches[plan.tasks[t].b].mpo, MpoAlgorithm::ZipUp, true, opt);
    } else {
        // Naive: the site products of all tasks and all sites in one launch, projection folded in; then the compress stage per task
        std::vector<std::vector<DevCore>> cores(nt);
        for (auto& c : cores) c.resize(n);
        std::vector<PmpoPairJob> jobs;
        jobs.reserve(nt * n);
        unsigned long long off = 0;
        for (size_t t = 0; t < nt; ++t)
            for (size_t i = 0; i < n; ++i) {
                jobs.push_back(pair_job(patches[plan.tasks[t].a], other.patches[plan.tasks[t].b], sd, other.sd, t, i, cores[t][i], off));
                off += cores[t][i].size();
            }
        launch_pairs(eng, jobs, off);
        if (compress && compress_route != CompressRoute::Serial) { // every task product in one call (batch_compress.hpp)
            std::vector<std::vector<DevCore>*> chains;
            for (auto& c : cores) chains.push_back(&c);
            compress_many_cores(eng, chains, opt, compress_route, nullptr);
        }
        for (size_t t = 0; t < nt; ++t) {
            if (compress && compress_route == CompressRoute::Serial) mpo_compress_cores(eng, cores[t], opt);
            products[t] = std::make_unique<Mpo>(std::move(cores[t]), rsd);
        }
    }
    // the first result with a new projector is inserted, a later one is added to it and truncated (partitioned_tt.rs:312-336); Naive
    // without compression keeps the exact direct sum, as contract_naive(a, b, None) keeps the exact product
    std::vector<std::unique_ptr<Mpo>> sums(plan.results.size());
    const bool trunc = (alg == MpoAlgorithm::ZipUp || compress) && truncates(opt);
    for (size_t t = 0; t < nt; ++t) {
        std::unique_ptr<Mpo>& slot = sums[plan.tasks[t].result];
        if (!slot) slot = std::move(products[t]);
        else slot = add_truncate(*slot, *products[t], trunc, opt);
    }
    for (size_t r = 0; r < sums.size(); ++r) out->patches.push_back({plan.results[r], std::move(sums[r])});
    return out;
}

// ------------------------------------------------------------------------------------------------ hooks
void pmpo_time_contract(PartitionedMpo& a, PartitionedMpo& b, const MpoContractionOptions& opt, size_t reps, double ms[3])
{
    check_operands(a, b);
    if (reps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "pmpo_time_contract: reps must be positive");
    const PmpoPlan plan = pmpo_contract_plan(projectors_of(a), projectors_of(b));
    if (plan.tasks.empty() || a.sd.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "pmpo_time_contract: the operands have no task");
    const size_t n = a.sd.size(), nt = plan.tasks.size();
    Engine& eng = a.patches[plan.tasks[0].a].mpo->tt.eng;
    sync_all(a);
    sync_all(b);
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    // [0] the fused launch (job upload included, as contract() pays it)
    std::vector<std::vector<DevCore>> cores(nt);
    for (auto& c : cores) c.resize(n);
    std::vector<PmpoPairJob> jobs;
    unsigned long long off = 0;
    for (size_t t = 0; t < nt; ++t)
        for (size_t i = 0; i < n; ++i) {
            jobs.push_back(pair_job(a.patches[plan.tasks[t].a], b.patches[plan.tasks[t].b], a.sd, b.sd, t, i, cores[t][i], off));
            off += cores[t][i].size();
        }
    launch_pairs(eng, jobs, off); // warm-up
    clk::time_point t0 = clk::now();
    for (size_t r = 0; r < reps; ++r) launch_pairs(eng, jobs, off);
    ms[0] = since(t0) / reps;
    // [1] the composition: mask copies of the operands in one launch, then one mpo_site_contract launch per task
    MpoContractionOptions none;
    auto composition = [&] {
        std::vector<std::unique_ptr<Mpo>> ca, cb;
        std::vector<std::vector<DevCore>*> chains;
        std::vector<const LegProjector*> projs;
        for (auto& q : a.patches) ca.push_back(std::make_unique<Mpo>(clone_cores(q.mpo->tt.cores, eng.stream()), a.sd));
        for (auto& q : b.patches) cb.push_back(std::make_unique<Mpo>(clone_cores(q.mpo->tt.cores, eng.stream()), b.sd));
        for (size_t k = 0; k < ca.size(); ++k) chains.push_back(&ca[k]->tt.cores), projs.push_back(&a.patches[k].proj);
        mask_chains(eng, chains, projs, a.sd);
        chains.clear();
        projs.clear();
        for (size_t k = 0; k < cb.size(); ++k) chains.push_back(&cb[k]->tt.cores), projs.push_back(&b.patches[k].proj);
        mask_chains(eng, chains, projs, b.sd);
        for (size_t t = 0; t < nt; ++t) mpo_contract(*ca[plan.tasks[t].a], *cb[plan.tasks[t].b], MpoAlgorithm::Naive, false, none);
    };
    composition(); // warm-up
    t0 = clk::now();
    for (size_t r = 0; r < reps; ++r) composition();
    ms[1] = since(t0) / reps;
    // [2] the compress stage of every task on copies of the products (the copies are outside the clock)
    double total = 0.0;
    for (size_t r = 0; r < reps + 1; ++r) {
        std::vector<std::vector<DevCore>> copy(nt);
        for (size_t t = 0; t < nt; ++t) copy[t] = clone_cores(cores[t], eng.stream());
        eng.sync();
        t0 = clk::now();
        for (size_t t = 0; t < nt; ++t) mpo_compress_cores(eng, copy[t], opt);
        if (r) total += since(t0); // the first round warms up
    }
    ms[2] = total / reps;
}

void pmpo_time_compress(PartitionedMpo& a, PartitionedMpo& b, const MpoContractionOptions& opt, size_t reps, double ms[2])
{
    check_operands(a, b);
    const PmpoPlan plan = pmpo_contract_plan(projectors_of(a), projectors_of(b));
    if (plan.tasks.empty() || a.sd.empty()) throw Error(T4A_GPU_INVALID_ARGUMENT, "pmpo_time_compress: the operands have no task");
    const size_t n = a.sd.size(), nt = plan.tasks.size();
    Engine& eng = a.patches[plan.tasks[0].a].mpo->tt.eng;
    sync_all(a);
    sync_all(b);
    std::vector<std::vector<DevCore>> cores(nt);
    for (auto& c : cores) c.resize(n);
    std::vector<PmpoPairJob> jobs;
    unsigned long long off = 0;
    for (size_t t = 0; t < nt; ++t)
        for (size_t i = 0; i < n; ++i) {
            jobs.push_back(pair_job(a.patches[plan.tasks[t].a], b.patches[plan.tasks[t].b], a.sd, b.sd, t, i, cores[t][i], off));
            off += cores[t][i].size();
        }
    launch_pairs(eng, jobs, off);
    compress_many_time(eng, cores, opt, reps, ms);
}

void pmpo_pair_products(const size_t* dims, const long long* sel, size_t n_jobs, const double* A, const double* B, double* C)
{
    if (n_jobs == 0) return;
    if (!dims || !sel || !A || !B || !C) throw Error(T4A_GPU_NULL_POINTER, "pair_products: null argument");
    if (n_jobs > (size_t)INT_MAX) throw Error(T4A_GPU_INVALID_ARGUMENT, "pair_products: more than INT_MAX jobs");
    std::vector<PmpoPairJob> jobs(n_jobs);
    size_t na = 0, nb = 0;
    unsigned long long nc = 0;
    for (size_t q = 0; q < n_jobs; ++q) {
        const size_t* d = dims + 7 * q;
        const long long* s = sel + 4 * q;
        const std::string where = "pair_products: job " + std::to_string(q);
        for (int x = 0; x < 7; ++x)
            if (d[x] == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, where + " has a zero dimension");
        check_site_count(d[0], d[1], d[2], d[3], where + ", A");
        check_site_count(d[4], d[2], d[5], d[6], where + ", B");
        check_site_count(d[0] * d[4], d[1], d[5], d[3] * d[6], where + ", C");
        if (s[0] < 0 || s[0] > s[1] || s[1] > (long long)d[2]) throw Error(T4A_GPU_INVALID_ARGUMENT, where + ": [k0, k1) is not inside [0, k)");
        if (s[2] >= (long long)d[1] || s[3] >= (long long)d[5]) throw Error(T4A_GPU_INVALID_ARGUMENT, where + ": a mask is out of range");
        PmpoPairJob& j = jobs[q];
        j = PmpoPairJob{};
        j.off = nc;
        j.la = (int)d[0], j.s1 = (int)d[1], j.k = (int)d[2], j.ra = (int)d[3], j.lb = (int)d[4], j.t = (int)d[5], j.rb = (int)d[6];
        j.k0 = (int)s[0], j.k1 = (int)s[1], j.sm = s[2] < 0 ? -1 : (int)s[2], j.tm = s[3] < 0 ? -1 : (int)s[3];
        na += d[0] * d[1] * d[2] * d[3];
        nb += d[4] * d[2] * d[5] * d[6];
        nc += (unsigned long long)(d[0] * d[4]) * d[1] * d[5] * (d[3] * d[6]);
    }
    require_device();
    Engine eng;
    DevBuf<double> da, db, dc;
    da.reserve(na);
    db.reserve(nb);
    dc.reserve(nc);
    T4A_HIP(hipMemcpyAsync(da.get(), A, na * sizeof(double), hipMemcpyHostToDevice, eng.stream()));
    T4A_HIP(hipMemcpyAsync(db.get(), B, nb * sizeof(double), hipMemcpyHostToDevice, eng.stream()));
    size_t oa = 0, ob = 0;
    for (size_t q = 0; q < n_jobs; ++q) {
        const size_t* d = dims + 7 * q;
        jobs[q].A = da.get() + oa;
        jobs[q].B = db.get() + ob;
        jobs[q].C = dc.get() + jobs[q].off;
        oa += d[0] * d[1] * d[2] * d[3];
        ob += d[4] * d[2] * d[5] * d[6];
    }
    launch_pairs(eng, jobs, nc);
    T4A_HIP(hipMemcpyAsync(C, dc.get(), nc * sizeof(double), hipMemcpyDeviceToHost, eng.stream()));
    eng.sync();
}

void pmpo_mask_sites(const size_t* dims, const long long* sel, size_t n_jobs, double* X)
{
    if (n_jobs == 0) return;
    if (!dims || !sel || !X) throw Error(T4A_GPU_NULL_POINTER, "mask_sites: null argument");
    SiteDims sd(n_jobs);
    LegProjector proj;
    for (size_t q = 0; q < n_jobs; ++q) {
        const size_t* d = dims + 4 * q;
        const std::string where = "mask_sites: job " + std::to_string(q);
        for (int x = 0; x < 4; ++x)
            if (d[x] == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, where + " has a zero dimension");
        check_site_count(d[0], d[1], d[2], d[3], where);
        sd[q] = {d[1], d[2]};
        if (sel[2 * q] >= 0) proj[{q, 0}] = (size_t)sel[2 * q];
        if (sel[2 * q + 1] >= 0) proj[{q, 1}] = (size_t)sel[2 * q + 1];
    }
    projector_validate(proj, sd);
    require_device();
    Engine eng;
    // the jobs are the sites of one chain here: job q is site q, bonds as given (they need not match)
    std::vector<DevCore> chain(n_jobs);
    size_t off = 0;
    for (size_t q = 0; q < n_jobs; ++q) {
        const size_t* d = dims + 4 * q;
        chain[q] = DevCore::make(d[0], d[1] * d[2], d[3]);
        T4A_HIP(hipMemcpyAsync(chain[q].buf.get(), X + off, chain[q].size() * sizeof(double), hipMemcpyHostToDevice, eng.stream()));
        off += chain[q].size();
    }
    mask_chains(eng, {&chain}, {&proj}, sd);
    off = 0;
    for (size_t q = 0; q < n_jobs; ++q) {
        T4A_HIP(hipMemcpyAsync(X + off, chain[q].buf.get(), chain[q].size() * sizeof(double), hipMemcpyDeviceToHost, eng.stream()));
        off += chain[q].size();
    }
    eng.sync();
}

} // namespace t4a
