// tci2_fill.hip — fill_site_tensors of the TensorCI2 driver (tensorci2.rs:1065-1186) and everything around it: the accumulators built
// ahead, planning and staging of a fill, its issue (directly or as a replayed HIP graph), fill_wait, the pending fill of optimize()
// and the asynchronous export / import of site tensors.
//
// All sites are independent given the final I/J sets, so the evaluations, the partial-pivot LU factorisations and the triangular
// solves of every site are issued as batches.  The whole fill runs on its own stream.  With `async` (optimize loop, nsearch == 0,
// built-in functor) the host does not wait: the next half-sweep's bond updates only need the index sets, so the fill overlaps with
// them (the rrLU chain leaves most CUs idle).  Errors (singular pivot matrix) surface at the next fill_wait().
//
// The stream operations of a fill are DATA (FillRecords, tci2.hpp): fill_issue() reads nothing else, so the records are also the
// key of the captured graph — a value an operation depends on cannot be missing from the key.
#include "tci2.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>

namespace t4a {

namespace {

// all cores of one fill_site_tensors in a single launch (blockIdx.y = site job; PackJob: kernels.hpp)
__global__ void __launch_bounds__(256) pack_fill_batched_kernel(const PackJob* __restrict__ jobs)
{
    const PackJob j = jobs[blockIdx.y];
    const size_t total = (size_t)j.L * j.S * j.R;
    const bool zero = j.info && *j.info == -1; // numerically zero pivot matrix: zero core (tensorci2.rs:1154-1157)
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int l = (int)(e % j.L);
        const int s = (int)((e / j.L) % j.S);
        const int r = (int)(e / ((size_t)j.L * j.S));
        if (j.last)
            j.core[e] = j.src[(size_t)r * j.ld + (l * j.S + s)]; // Pi1 itself (tensorci2.rs:1109-1128), R == 1
        else
            j.core[e] = zero ? 0.0 : j.src[(size_t)(l * j.S + s) * j.ld + r]; // (tensorci2.rs:1167-1181)
    }
}

enum : unsigned { FILL_ZEROS = 1, FILL_FLAGS = 2, FILL_SOLVE = 4, FILL_ALL = 7 };

// Issues the operations the records describe on `st`, in order: the all-zero cores, the zeroing of the flags, then the upload, the
// evaluations (built-in functor), the batched solve, the packing and the copy-back of the solve status.
void fill_issue(const FillRecords& rec, unsigned parts, hipStream_t st)
{
    const FillOps& o = rec.ops;
    if (parts & FILL_ZEROS)
        for (const FillZero& z : rec.zeros) fill_launch(z.ptr, z.count, 0.0, st);
    if (parts & FILL_FLAGS) T4A_HIP(hipMemsetAsync(o.flags, 0, o.flag_bytes, st));
    if (!(parts & FILL_SOLVE)) return;
    T4A_HIP(hipMemcpyAsync(o.stage_dev, o.stage_host, o.stage_bytes, hipMemcpyHostToDevice, st));
    if (o.small) {
        // small problems (BASELINE configs[1], the first iterations of every run): evaluation, solve and packing of all sites in ONE
        // launch (fill_small_kernel) instead of five dependent ones — bitwise the same cores
        fill_small_launch(o.fn, o.pis, o.lups, o.packs, o.n_site_jobs, o.last_site, st);
        T4A_HIP(hipMemcpyAsync(o.info_host, o.info_dev, o.info_bytes, hipMemcpyDeviceToHost, st));
        return;
    }
    // (1) evaluations.  B_b = Pi1^T (nj x ni), A_b = P^T (nj x np) — evaluated directly in transposed form
    //     (solve(P^T, Pi1^T), tensorci2.rs:1160-1162).  A host callback has evaluated them already (n_pi == 0).
    if (o.n_pi) pi_eval_batched_launch(o.fn, o.pis, o.n_pi, o.max_M, o.max_N, st);
    // (2) batched solve; the zero-pivot-matrix guard (:1154-1157) is evaluated on the device: lu_kernel reads
    //     max|P| and flags info = -1, the solves skip flagged problems and the packing writes a zero core
    if (o.n_lu) {
        // one fused solve behind the blocked LU of the pivot matrices; outside its size range the blocked LU with the unit-lower
        // forward substitution folded in; beyond that one's limit the unblocked kernel + explicit forward solve (bitwise the same)
        if (!lu_solve_blocked_launch(o.lups, o.n_lu, o.max_n, o.max_nrhs, st, o.avoid_xcc, o.tickets)) {
            if (!lu_forward_blocked_launch(o.lups, o.n_lu, o.max_n, o.max_nrhs, st, o.avoid_xcc, o.tickets)) {
                lu_batched_launch(o.lups, o.n_lu, o.max_n, st);
                trsm_left_batched_launch(o.trs, o.n_lu, o.max_n, o.max_nrhs, st);
            }
            trsm_left_batched_launch(o.trs + o.n_lu, o.n_lu, o.max_n, o.max_nrhs, st);
        }
    }
    // (3) pack all cores in one launch
    hipLaunchKernelGGL(pack_fill_batched_kernel, dim3(o.pack_gx, o.pack_gy), dim3(256), 0, st, o.packs);
    T4A_HIP(hipMemcpyAsync(o.info_host, o.info_dev, o.info_bytes, hipMemcpyDeviceToHost, st));
}

// one site of a fill that has something to solve or evaluate
struct SiteJob {
    size_t b;
    size_t ni, nj, np;
    size_t offA, offB;       // offsets (doubles) into fill_.A / fill_.B ...
    double *A, *B;           // ... and the addresses, once the buffers have their size: P^T (null for the last site), Pi1^T
    unsigned long long* pmax; // max|P| bits of the site
    size_t accJ, accK, accI; // offsets (u64) into the accumulator arena: J_b, kron_i(b), I_{b+1}
    bool last;
};
// the job tables of a fill beside the Π jobs, one entry per solved site (packs: per site)
struct FillTables {
    std::vector<LuProblem> lups;
    std::vector<TrsmProblem> trl, tru; // unit-lower and upper solve of every LU problem
    std::vector<PackJob> packs;
};

// T4A_HOST_PROFILE: host time of fill_site_tensors by phase, microseconds summed over all calls of the process (tools/probe_cfg2_host.py)
struct HostProfile {
    const bool on = std::getenv("T4A_HOST_PROFILE") != nullptr;
    double wait_jobs = 0, descriptors = 0, accumulators = 0, staging = 0, issue = 0; // the phases of a call, in order
    double reserve = 0, acc_copy = 0, job_tables = 0;                                // staging in detail (not part of `staging`)
    double total = 0;
    long calls = 0;
} g_prof;
struct HostLap { // adds the time since the last lap to one phase
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t = t0;
    void operator()(double& phase)
    {
        if (!g_prof.on) return;
        const auto now = std::chrono::steady_clock::now();
        phase += std::chrono::duration<double, std::micro>(now - t).count();
        t = now;
    }
};

// the legacy default stream, or a blocking stream (which orders against it exactly like it): no graph replay beside these
bool stream_orders_with_legacy(hipStream_t s)
{
    if (s == nullptr) return true;
    unsigned flags = 0;
    if (hipStreamGetFlags(s, &flags) != hipSuccess) {
        (void)hipGetLastError();
        return true; // (unknown: the careful answer)
    }
    return (flags & hipStreamNonBlocking) == 0;
}

// Lays out [accumulators | Π jobs | LU problems | triangular solves (lower, then upper) | packing jobs] in the pinned staging buffer
// and enters the copy and the device addresses of the tables into `ops`: ONE host-to-device copy carries all of it.  with_pi
// (built-in functor): `acc` holds the accumulators of all jobs (SiteJob::accJ / accK / accI point into it) and the Π jobs are built
// from them; without (host callback: the matrices are evaluated already) `acc` is empty and there are no Π jobs.
void fill_stage(PinBuf<uint64_t>& hstage, DevBuf<uint64_t>& dstage, const std::vector<SiteJob>& jobs, const std::vector<uint64_t>& acc,
                bool with_pi, const FillTables& tab, FillOps& ops, HostLap& lap)
{
    const std::vector<LuProblem>& lups = tab.lups;
    const std::vector<PackJob>& packs = tab.packs;
    auto up8 = [](size_t v) { return (v + 7) / 8 * 8; };
    const size_t np = lups.size(), n_pi_slots = with_pi ? 2 * jobs.size() : 0;
    const size_t bytes_acc = acc.size() * sizeof(uint64_t), bytes_lu = np * sizeof(LuProblem), bytes_tr = np * sizeof(TrsmProblem);
    const size_t bytes_pk = packs.size() * sizeof(PackJob);
    const size_t off_pi = up8(bytes_acc), off_lu = up8(off_pi + n_pi_slots * sizeof(PiJob));
    const size_t off_tr = up8(off_lu + bytes_lu), off_pk = up8(off_tr + 2 * bytes_tr);
    const size_t total_bytes = up8(off_pk + bytes_pk);
    hstage.reserve(total_bytes / 8);
    dstage.reserve(total_bytes / 8);
    lap(g_prof.reserve);
    char* hb = reinterpret_cast<char*>(hstage.get());
    char* db = reinterpret_cast<char*>(dstage.get());
    if (bytes_acc) std::memcpy(hb, acc.data(), bytes_acc);
    lap(g_prof.acc_copy);
    if (n_pi_slots) {
        const uint64_t* da = dstage.get();
        std::vector<PiJob> pis;
        for (const SiteJob& j : jobs) {
            PiJob q{};
            q.out = j.B;
            if (j.last) { // last site stores Pi1 itself (:1109-1128): ni x nj
                q.rowacc = da + j.accK;
                q.M = (int)j.ni;
                q.colacc = da + j.accJ;
                q.N = (int)j.nj;
                q.ld = (int)j.ni;
                pis.push_back(q);
            } else {
                q.rowacc = da + j.accJ;
                q.M = (int)j.nj;
                q.colacc = da + j.accK;
                q.N = (int)j.ni;
                q.ld = (int)j.nj;
                pis.push_back(q);
                q.colacc = da + j.accI;
                q.N = (int)j.np;
                q.out = j.A;
                q.max_abs_bits = j.pmax;
                pis.push_back(q);
            }
        }
        for (const PiJob& q : pis) {
            ops.max_M = std::max(ops.max_M, q.M);
            ops.max_N = std::max(ops.max_N, q.N);
        }
        std::memcpy(hb + off_pi, pis.data(), pis.size() * sizeof(PiJob));
        ops.pis = reinterpret_cast<const PiJob*>(db + off_pi);
        ops.n_pi = (int)pis.size();
    }
    if (np) {
        std::memcpy(hb + off_lu, lups.data(), bytes_lu);
        std::memcpy(hb + off_tr, tab.trl.data(), bytes_tr);
        std::memcpy(hb + off_tr + bytes_tr, tab.tru.data(), bytes_tr);
    }
    std::memcpy(hb + off_pk, packs.data(), bytes_pk);
    lap(g_prof.job_tables);
    ops.stage_dev = db;
    ops.stage_host = hb;
    ops.stage_bytes = total_bytes;
    ops.lups = reinterpret_cast<const LuProblem*>(db + off_lu);
    ops.trs = reinterpret_cast<const TrsmProblem*>(db + off_tr);
    ops.packs = reinterpret_cast<const PackJob*>(db + off_pk);
}

} // namespace

void Tci2::invalidate_fill_cache()
{
    for (auto& f : fill_.cache) f.valid = false;
}

// Accumulators fill_site_tensors needs for site b (tensorci2.rs:1101-1145): J_b, kron(I_b, d_b) and I_{b+1}.
void Tci2::prepare_fill_site(size_t b)
{
    if (!fn_.builtin() || b >= n_) return;
    if (chain_.digits_stale) { // after a bond chain the accumulators are in the pinned mirror of the device tables: no digits needed
        prepare_fill_site_from_mirror(b);
        return;
    }
    if (fill_.cache.size() != n_) fill_.cache.assign(n_, FillAcc());
    if (shard_world > 1 && (b % shard_world) != shard_rank) return;
    FillAcc& f = fill_.cache[b];
    f.valid = false;
    if (i_set[b].count == 0 || j_set[b].count == 0) return;
    accumulate(j_set[b], b + 1, f.accJ);
    accumulate(kronecker_i(b), 0, f.accK);
    if (b + 1 < n_)
        accumulate(i_set[b + 1], 0, f.accI);
    else
        f.accI.clear();
    f.valid = true;
}

// optimize() with bounded rank and a built-in functor: site tensors and fill workspaces get their final size now (a buffer that
// grows goes through the process-wide cache, which waits for the whole device: once per iteration and buffer while ranks grow)
void Tci2::fill_presize(const TCI2Options& options)
{
    if (!fn_.builtin() || options.max_bond_dim == 0 || options.max_bond_dim > 1024) return;
    const size_t chi = options.max_bond_dim;
    // what a bond can reach at all: min(chi, product of the local dimensions on either side) — the ends of a train stay small
    std::vector<size_t> lb(n_ + 1, 1), rb(n_ + 1, 1);
    for (size_t b = 0; b < n_; ++b) lb[b + 1] = std::min(chi, lb[b] * local_dims[b]);
    for (size_t b = n_; b-- > 0;) rb[b] = std::min(chi, rb[b + 1] * local_dims[b]);
    auto bond = [&](size_t b) { return std::min(lb[b], rb[b]); }; // bond b sits left of site b
    auto mine = [&](size_t b) { return shard_world <= 1 || (b % shard_world) == shard_rank; };
    size_t totA = 0, totB = 0, tot_cores = 0, acc_words = 0;
    for (size_t b = 0; b < n_; ++b) {
        if (!mine(b)) continue;
        const size_t l = bond(b), rr = bond(b + 1);
        tot_cores += l * local_dims[b] * rr;
        totA += rr * rr;
        totB += rr * l * local_dims[b];
        acc_words += chi * (2 + local_dims[b]) * (size_t)fn_.dev.n_acc;
    }
    // ... and only while the whole reservation stays moderate (chi = 1024 over 100 sites is 4 GB per handle,
    // times eight handles of a group, for a run that may stay at rank 10): beyond that the buffers grow on demand as before
    if ((tot_cores + totA + totB) * sizeof(double) > ((size_t)1 << 30)) return;
    for (size_t b = 0; b < n_; ++b)
        if (mine(b)) cores[b].buf.reserve(std::max<size_t>(bond(b) * local_dims[b] * bond(b + 1), 1));
    fill_.A.reserve(std::max<size_t>(totA, 1));
    fill_.B.reserve(std::max<size_t>(totB, 1));
    fill_.piv.reserve(std::max<size_t>(n_ * chi, 1));
    // the upload arena of a fill (accumulators of J_b, kron(I_b, d_b), I_{b+1} per site, then the job tables): grown once
    // per iteration it cost every fill a device-wide wait in the middle of the next chain
    const size_t desc_bytes = n_ * (2 * sizeof(PiJob) + sizeof(LuProblem) + 2 * sizeof(TrsmProblem) + 64) + 256;
    fill_.hstage.reserve(acc_words + desc_bytes / 8 + 64);
    fill_.dstage.reserve(acc_words + desc_bytes / 8 + 64);
    fill_.flags.reserve(n_ + (n_ + 1) / 2 + (LU_MAX_PANEL_STEPS + 1) / 2);
    fill_.hinfo.reserve(n_);
}

void Tci2::fill_site_tensors() { fill_run(FillOptions()); }

// Issues the stream operations of one fill.  Fills of consecutive sweeps at saturated rank are operation-for-operation
// identical (same device addresses, shapes and pinned staging buffer), so the sequence is captured into a HIP graph the
// second time its records are seen and replayed afterwards: one submission instead of ~25, which also keeps the
// runtime's submission path free for the latency-critical bond updates on the main stream.
void Tci2::issue_fill_ops(const FillRecords& rec)
{
    hipStream_t st = fill_.stream;
    static const bool use_graph = std::getenv("T4A_NO_FILL_GRAPH") == nullptr;
    if (fill_.timed) T4A_HIP(hipEventRecord(fill_.ev.a, st));
    bool done = false;
    // (no graph replay on a handle whose cores are exported / imported through the LEGACY DEFAULT STREAM.  Round 4 saw GPU memory
    // faults in 25 - 75 % of `bench.py --mode site-shard` runs with replay on; round 5 bisected them (tools/r5_gpu_shardfault*.sh,
    // profiles/r05_fill_graph_fault_bisect.txt, five runs per arm): they need the replay AND an event protocol that runs through
    // stream 0 — torch's current stream in a process that never selected another — in BOTH directions (export: stream 0 waits for an
    // event recorded behind the replay; import: the import stream waits for an event recorded on stream 0).  Replacing either event
    // by a host wait, moving torch to a side stream, or a device-wide synchronisation in front of the replay: 0 faults of 5; the
    // pool, the bond chain, kernel serialisation, the order of the export copies and the copy nodes of the graph: no influence.
    // Every pointer the graph holds is part of the signature (checked again: tables, staging buffers, tickets, flags), so this is
    // the runtime's implicit ordering of stream 0 against the streams a graph launch runs on, not a stale pointer.  parallel.py and
    // bench.py therefore exchange on a side stream; a caller that hands in stream 0 gets direct issue, which is what the
    // round-4 stop-gap did for every shared handle.)
    // the root cause is NOT identified (the library's streams are non-blocking, so "implicit ordering with stream 0"
    // does not explain the faults, and no multi-GPU soak of the patch-farm path exists).  The default is therefore the round-4 guard —
    // no replay on ANY handle whose site tensors are exported / imported asynchronously; the relaxed guard (replay unless the legacy
    // stream or a blocking stream took part) is an opt-in: t4a_gpu_tci2_set_chain bit 4.  The gain it buys is ~0.4 % of a sweep.
    const bool shared_ok = !fill_.cores_shared_async || (fill_graph_relaxed && !fill_.cores_shared_legacy_stream);
    if (use_graph && !fill_.graph_broken && shared_ok) {
        if (fill_.graph_exec && rec == fill_.graph) {
            T4A_HIP(hipGraphLaunch(fill_.graph_exec, st));
            ++fill_.stats[1];
            done = true;
        } else if (rec == fill_.last) { // second time in a row: worth capturing
            if (fill_.graph_exec) {
                (void)hipGraphExecDestroy(fill_.graph_exec);
                fill_.graph_exec = nullptr;
            }
            hipGraph_t graph = nullptr;
            pool::capture_begin(); // (no device-wide synchronisation of another handle's thread may fall into the capture)
            bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                try {
                    fill_issue(rec, FILL_ALL, st);
                } catch (...) {
                    ok = false;
                }
                if (hipStreamEndCapture(st, &graph) != hipSuccess || !graph) ok = false;
            }
            pool::capture_end();
            if (ok && hipGraphInstantiate(&fill_.graph_exec, graph, nullptr, nullptr, 0) != hipSuccess) {
                fill_.graph_exec = nullptr;
                ok = false;
            }
            if (graph) (void)hipGraphDestroy(graph);
            if (ok) {
                fill_.graph = rec;
                T4A_HIP(hipGraphLaunch(fill_.graph_exec, st));
                ++fill_.stats[2];
                done = true;
            } else {
                (void)hipGetLastError();
                fill_.graph_broken = true; // never try again on this handle; fall through to the direct issue
            }
        }
    }
    fill_.last = rec;
    ++fill_.stats[0];
    if (!done) fill_issue(rec, FILL_ALL, st);
    if (fill_.timed) T4A_HIP(hipEventRecord(fill_.ev.b, st));
}

void Tci2::fill_wait()
{
    if (fill_.import_inflight) { // cores of the other ranks' sites (site-sharded fill) still on their way into this handle
        fill_.import_inflight = false;
        T4A_HIP(hipStreamSynchronize(fill_.import_stream));
    }
    if (!fill_.inflight) return;
    fill_.inflight = false;
    T4A_HIP(hipStreamSynchronize(fill_.stream));
    T4A_HIP(hipGetLastError());
    if (eng.prof.enabled && fill_.timed) {
        float ms = 0.f;
        T4A_HIP(hipEventElapsedTime(&ms, fill_.ev.a, fill_.ev.b));
        eng.prof.v[4] += ms;
        eng.prof.v[5] += 1.0;
    }
    fill_.timed = false;
    for (size_t k = 0; k < fill_.solved_sites.size(); ++k)
        if (fill_.hinfo.get()[fill_.solved_sites[k]] > 0) {
            const size_t site = fill_.solved_sites[k];
            fill_.solved_sites.clear();
            throw Error(T4A_GPU_INTERNAL_ERROR, "one-site interpolation solve failed: singular pivot matrix at site " +
                                                    std::to_string(site));
        }
    fill_.solved_sites.clear();
}

void Tci2::fill_run(FillOptions opt)
{
    fn_.require("tci2");
    HostLap lap;
    // accumulators built ahead are only trusted when optimize() vouches for them (same half-sweep, sets final)
    if (!opt.trust_cache) invalidate_fill_cache();
    const bool builtin = fn_.builtin();
    if (!builtin) sync_digits();
    fill_wait(); // the scratch arenas of the previous fill are free again
    if (!fill_.stream) fill_.stream = pool::stream_get(2); // lowest priority, recycled through the process-wide cache
    static const bool sync_fill = std::getenv("T4A_SYNC_FILL") != nullptr; // measurement switch: no overlap at all
    if (!builtin || sync_fill) opt.async = false;
    // everything of this fill is ordered after the work already enqueued on the main stream (the per-bond path writes site
    // tensors there).  After a bond chain nothing on the main stream concerns the fill — and the NEXT chain may already be
    // running on it: no wait then.
    const bool no_main_sync = opt.no_main_sync && builtin;
    if (!no_main_sync) T4A_HIP(hipStreamSynchronize(eng.stream()));
    hipStream_t st = fill_.stream;
    FillRecords rec; // the stream operations of this fill (no event records)
    FillOps& ops = rec.ops;
    std::vector<SiteJob> jobs;
    size_t totA = 0, totB = 0;
    for (size_t b = 0; b < n_; ++b) {
        if (shard_world > 1 && (b % shard_world) != shard_rank) continue;
        const size_t ni = i_set[b].count * local_dims[b];
        const size_t nj = j_set[b].count;
        if (ni == 0 || nj == 0) { // tensorci2.rs:1074-1092
            const size_t left_dim = (b == 0) ? 1 : std::max<size_t>(i_set[b].count, 1);
            const size_t right_dim = (b == n_ - 1) ? 1 : std::max<size_t>(i_set[b + 1].count, 1);
            DevCore& c = cores[b];
            c.reshape(left_dim, local_dims[b], right_dim);
            rec.zeros.push_back(FillZero{c.buf.get(), c.size()});
            continue;
        }
        SiteJob j;
        j.b = b;
        j.ni = ni;
        j.nj = nj;
        j.last = (b == n_ - 1);
        j.np = j.last ? 0 : i_set[b + 1].count;
        if (!j.last && j.np != nj)
            throw Error(T4A_GPU_INTERNAL_ERROR, "one-site interpolation solve failed: pivot matrix at bond " +
                                                    std::to_string(b) + " is not square (" + std::to_string(j.np) + " x " +
                                                    std::to_string(nj) + ")");
        j.offA = totA;
        j.offB = totB;
        j.accJ = j.accK = j.accI = 0;
        totA += j.last ? 0 : nj * j.np;
        totB += nj * ni;
        jobs.push_back(j);
    }
    lap(g_prof.wait_jobs);
    if (jobs.empty()) {
        fill_issue(rec, FILL_ZEROS, st);
        T4A_HIP(hipStreamSynchronize(st));
        return;
    }
    // host-callback mode stays immediate (its evaluations are synchronous anyway)
    if (!builtin) fill_issue(rec, FILL_ZEROS, st);
    fill_.A.reserve(std::max<size_t>(totA, 1));
    fill_.B.reserve(totB);
    // max|P| bits (n_ u64), solve status (n_ ints) and the work tickets of the trailing updates share one allocation -> one memset
    const size_t fm_words = n_ + (n_ + 1) / 2 + (LU_MAX_PANEL_STEPS + 1) / 2;
    fill_.flags.reserve(fm_words);
    unsigned long long* d_max = fill_.flags.get();
    int* d_info = reinterpret_cast<int*>(fill_.flags.get() + n_);
    fill_.hinfo.reserve(n_);
    ops.flags = fill_.flags.get();
    ops.flag_bytes = fm_words * sizeof(unsigned long long);
    ops.tickets = reinterpret_cast<unsigned*>(fill_.flags.get() + n_ + (n_ + 1) / 2);
    // beside a bond chain the fill keeps off the chain's XCD where it could not be placed anyway (lu_update_kernel)
    ops.avoid_xcc = (no_main_sync && !xcd_disabled()) ? eng.xcc() : -1;
    ops.info_dev = d_info;
    ops.info_host = fill_.hinfo.get();
    ops.info_bytes = n_ * sizeof(int);
    ops.fn = fn_.dev;
    fill_.timed = eng.prof.enabled;
    if (!builtin) {
        if (fill_.timed) T4A_HIP(hipEventRecord(fill_.ev.a, st));
        fill_issue(rec, FILL_FLAGS, st);
        // the callback evaluations below write max|P| on the MAIN stream: the zeroing must have landed before them, or a late
        // memset (queued behind other handles' fills, e.g. in fill_site_tensors_group) erases max|P| and the guard zeroes the core
        T4A_HIP(hipStreamSynchronize(st));
    }

    // core shapes are known up front: allocate them now so that every device address below is final
    size_t piv_total = 0;
    for (SiteJob& j : jobs) {
        j.A = j.last ? nullptr : fill_.A.get() + j.offA;
        j.B = fill_.B.get() + j.offB;
        j.pmax = d_max + j.b;
        DevCore& c = cores[j.b];
        c.reshape((j.b == 0) ? 1 : i_set[j.b].count, local_dims[j.b], j.last ? 1 : j.np);
        piv_total += j.np;
    }
    fill_.piv.reserve(std::max<size_t>(piv_total, 1));

    // solve descriptors (device addresses only): built before the upload so that ONE host-to-device copy carries
    // the accumulators, the evaluation jobs, the LU / triangular-solve problems and the packing jobs
    FillTables tab;
    size_t piv_off = 0, max_core = 1;
    fill_.solved_sites.clear();
    double flops = 0.0;
    // small problems: one launch (fill_issue).  Only with a built-in functor, and only when every site fits
    ops.small = builtin;
#ifdef T4A_TEST_HOOKS
    // libt4a_gpu_testhooks.so only: the general five-launch path for small problems too, so that a test can compare the two bit by bit
    // (tests/test_gpu_tci2.py::test_small_problem_fill_in_one_launch_is_bitwise_the_general_path)
    if (std::getenv("T4A_TEST_NO_SMALL_FILL")) ops.small = 0;
#endif
    for (const SiteJob& j : jobs) {
        if (j.nj > (size_t)FILL_SMALL_MAX_N || j.ni > (size_t)FILL_SMALL_MAX_RHS) ops.small = 0;
        const DevCore& c = cores[j.b];
        PackJob pk;
        pk.src = j.B;
        pk.core = c.buf.get();
        pk.L = (int)c.l;
        pk.S = (int)c.s;
        pk.R = (int)c.r;
        pk.last = j.last ? 1 : 0;
        pk.ld = j.last ? (int)j.ni : (int)j.nj;
        pk.info = j.last ? nullptr : (const int*)(d_info + j.b);
        pk.pad_ = 0;
        tab.packs.push_back(pk);
        max_core = std::max(max_core, c.size());
        if (j.last) continue;
        LuProblem lp;
        lp.A = j.A;
        lp.lda = (int)j.nj;
        lp.n = (int)j.nj;
        lp.piv = fill_.piv.get() + piv_off;
        lp.info = d_info + j.b;
        lp.B = j.B;
        lp.ldb = (int)j.nj;
        lp.nrhs = (int)j.ni;
        lp.pmax_bits = j.pmax;
        piv_off += j.np;
        tab.lups.push_back(lp);
        tab.trl.push_back(lu_trsm_problem(lp, true, lp.info));
        tab.tru.push_back(lu_trsm_problem(lp, false, lp.info));
        fill_.solved_sites.push_back(j.b);
        ops.max_n = std::max(ops.max_n, lp.n);
        ops.max_nrhs = std::max(ops.max_nrhs, lp.nrhs);
        const double n = (double)j.np;
        flops += (2.0 / 3.0) * n * n * n + 2.0 * n * n * (double)j.ni;
    }
    ops.n_lu = (int)tab.lups.size();
    ops.pack_gx = (unsigned)std::min<size_t>((max_core + 255) / 256, 64);
    ops.pack_gy = (unsigned)tab.packs.size();
    ops.n_site_jobs = (int)jobs.size();
    ops.last_site = jobs.back().last ? 1 : 0;
    lap(g_prof.descriptors);

    std::vector<uint64_t> acc_all;
    if (builtin) {
        const size_t Kacc = (size_t)fn_.dev.n_acc;
        for (SiteJob& j : jobs) {
            const bool cached = fill_.cache.size() == n_ && fill_.cache[j.b].valid &&
                                fill_.cache[j.b].accJ.size() == j.nj * Kacc && fill_.cache[j.b].accK.size() == j.ni * Kacc &&
                                (j.last || fill_.cache[j.b].accI.size() == j.np * Kacc);
            if (!cached) prepare_fill_site(j.b); // sites that became final only with the last bonds of the sweep
            const FillAcc& f = fill_.cache[j.b];
            j.accJ = acc_all.size();
            acc_all.insert(acc_all.end(), f.accJ.begin(), f.accJ.end());
            j.accK = acc_all.size();
            acc_all.insert(acc_all.end(), f.accK.begin(), f.accK.end());
            if (!j.last) {
                j.accI = acc_all.size();
                acc_all.insert(acc_all.end(), f.accI.begin(), f.accI.end());
            }
            eng.prof.v[11] += (double)j.ni * j.nj + (double)j.np * j.nj;
        }
        invalidate_fill_cache();
        lap(g_prof.accumulators);
    } else {
        // host callback: evaluated synchronously through eval_matrix (main stream), then continue on `st`
        for (const SiteJob& j : jobs) {
            IndexSet ik = kronecker_i(j.b);
            const IndexSet& jb = j_set[j.b];
            if (j.last) {
                eval_matrix(ik, 0, jb, ik.width, j.B, nullptr);
            } else {
                eval_matrix(jb, j.b + 1, ik, 0, j.B, nullptr);
                eval_matrix(jb, j.b + 1, i_set[j.b + 1], 0, j.A, j.pmax);
            }
        }
        T4A_HIP(hipStreamSynchronize(eng.stream()));
        acc_used_ = 0;
        lap(g_prof.staging); // (the evaluations count as staging in the host profile)
    }
    fill_stage(fill_.hstage, fill_.dstage, jobs, acc_all, builtin, tab, ops, lap);
    lap(g_prof.staging);
    eng.prof.v[10] += flops;
    if (!builtin) {
        fill_issue(rec, FILL_SOLVE, st);
        if (fill_.timed) T4A_HIP(hipEventRecord(fill_.ev.b, st));
    } else {
        issue_fill_ops(rec);
    }
    fill_.inflight = true;
    if (g_prof.on) {
        g_prof.total += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - lap.t0).count();
        lap(g_prof.issue);
        const HostProfile& p = g_prof;
        if (++g_prof.calls % 20 == 0) {
            const double c = (double)p.calls;
            std::fprintf(stderr, "[host profile] fill_site_tensors host part %.1f us per call (wait+jobs %.1f, descriptors %.1f, "
                                 "accumulators %.1f, staging %.1f, issue %.1f)\n",
                         p.total / c, p.wait_jobs / c, p.descriptors / c, p.accumulators / c, p.staging / c, p.issue / c);
            std::fprintf(stderr, "[host profile]   staging in detail: reserve %.1f, accumulator copy %.1f, job tables %.1f us per call\n",
                         p.reserve / c, p.acc_copy / c, p.job_tables / c);
        }
    }
    if (!opt.async) fill_wait();
}

// fill_site_tensors on several handles: issue all, then complete all (t4a_gpu_tci2_fill_site_tensors_group)
void Tci2::fill_site_tensors_group(const std::vector<Tci2*>& hs)
{
    for (Tci2* h : hs)
        if (!h) throw Error(T4A_GPU_NULL_POINTER, "fill_site_tensors_group: null handle");
    std::exception_ptr first_error;
    for (Tci2* h : hs) {
        try {
            h->fill_run(FillOptions{true}); // asynchronous for built-in functors (a host callback fills synchronously)
        } catch (...) {
            if (!first_error) first_error = std::current_exception();
        }
    }
    for (Tci2* h : hs) {
        try {
            h->fill_wait();
        } catch (...) {
            if (!first_error) first_error = std::current_exception();
        }
    }
    if (first_error) std::rethrow_exception(first_error);
}

// optimize(): while the device works on the bond chain of an iteration the host issues fill_site_tensors of the PREVIOUS one (its
// accumulators come from the mirror that iteration left; nothing of it touches the main stream); the last iteration's fill goes out
// behind the loop (opt_end).  A group calls this for every handle before it finishes (or waits for) the first one: the first
// chain_finish waits for the whole group's chain, and whatever the host issues after that no longer overlaps it.
void Tci2::opt_issue_pending_fill(OptRun& r)
{
    if (!r.pending_fill) return;
    r.pending_fill = false;
#ifdef T4A_TEST_HOOKS
    {   // libt4a_gpu_testhooks.so only (build.py; tests/test_gpu_chain.py loads it in a child process): T4A_TEST_THROW_IN_FILL=n makes
        // the n-th pending fill of the process fail while a chain is in flight.  The production library carries no fault injector.
        static const long inject_at = std::getenv("T4A_TEST_THROW_IN_FILL") ? std::atol(std::getenv("T4A_TEST_THROW_IN_FILL")) : 0;
        static std::atomic<long> issued{0};
        if (inject_at > 0 && ++issued == inject_at)
            throw Error(T4A_GPU_INTERNAL_ERROR, "injected failure while issuing fill_site_tensors (T4A_TEST_THROW_IN_FILL)");
    }
#endif
    for (size_t b = 0; b < n_; ++b) prepare_fill_site(b); // (from the mirror of the previous chain; the new one writes the other mirror)
    fill_run(FillOptions{true, true, true}); // asynchronous; the accumulators just built are current; nothing of it is on the main stream
    if (!keep_site_tensors) invalidate_site_tensors(); // (the end of that iteration invalidated them, tensorci2.rs:707-708)
}

// Copies the site tensors first, first + step, ... to d_dst + k * stride (doubles, k = 0, 1, ...) WITHOUT blocking the host: the
// copies are ordered after a fill that is still in flight (same stream) and `consumer` waits for them through an event.
void Tci2::export_cores_async(size_t first, size_t step, double* d_dst, size_t stride, hipStream_t consumer, const char* what)
{
    fill_.cores_shared_async = true;
    if (stream_orders_with_legacy(consumer)) fill_.cores_shared_legacy_stream = true; // (see issue_fill_ops)
    hipStream_t st = fill_.inflight ? fill_.stream : eng.stream();
    size_t k = 0;
    for (size_t s = first; s < n_; s += step, ++k) {
        const DevCore& c = cores[s];
        if (c.size() > stride) throw Error(T4A_GPU_BUFFER_TOO_SMALL, std::string(what) + ": stride smaller than a site tensor");
        if (c.size())
            T4A_HIP(hipMemcpyAsync(d_dst + k * stride, c.buf.get(), c.size() * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    if (!fill_.export_event) T4A_HIP(hipEventCreateWithFlags(&fill_.export_event, hipEventDisableTiming));
    T4A_HIP(hipEventRecord(fill_.export_event, st));
    T4A_HIP(hipStreamWaitEvent(consumer, fill_.export_event, 0));
}

// every site tensor, site s to d_dst + s * stride
void Tci2::export_site_tensors_async(double* d_dst, size_t stride, hipStream_t consumer)
{
    export_cores_async(0, 1, d_dst, stride, consumer, "export_site_tensors");
}

// Site-sharded fill (BASELINE.json configs[3]): the sites s = shard_rank + shard_world * k of this rank go to
// d_dst + k * stride on the stream of the fill that may still be in flight; `consumer` (the stream of the all-gather) waits.
void Tci2::export_site_shard_async(double* d_dst, size_t stride, hipStream_t consumer)
{
    export_cores_async(shard_rank, shard_world, d_dst, stride, consumer, "export_site_shard");
}

// The other ranks' cores out of the gathered buffer [world][per_rank][stride]: site s of rank r = s % world sits at
// (r * per_rank + s / world) * stride.  Shapes follow from the (replicated) index sets AS THEY ARE NOW: call this in the same
// half-sweep as the export on the other ranks (parallel.ShardedCoreExchange does), before the next bond update changes a
// bond dimension.  The copies run on the handle's import stream after everything `producer` (the all-gather's stream) has
// enqueued so far; nothing blocks the host, the local fill still in flight is not waited for (it writes other sites), and
// the first reader of a core (fill_wait) waits for the import.
void Tci2::import_site_shard_async(const double* d_src, size_t stride, size_t per_rank, hipStream_t producer)
{
    fill_.cores_shared_async = true;
    if (stream_orders_with_legacy(producer)) fill_.cores_shared_legacy_stream = true; // (see issue_fill_ops)
    if (!fill_.import_stream) fill_.import_stream = pool::stream_get(2);
    // at most one import in flight: the one of the previous half-sweep is long done (a whole chain of bond updates ago),
    // and with it every read of the receive buffer that the caller is about to reuse
    T4A_HIP(hipStreamSynchronize(fill_.import_stream));
    if (!fill_.import_event) T4A_HIP(hipEventCreateWithFlags(&fill_.import_event, hipEventDisableTiming));
    T4A_HIP(hipEventRecord(fill_.import_event, producer));
    T4A_HIP(hipStreamWaitEvent(fill_.import_stream, fill_.import_event, 0));
    for (size_t s = 0; s < n_; ++s) {
        const size_t r = s % shard_world;
        if (r == shard_rank) continue;
        DevCore& c = cores[s];
        const size_t l = (s == 0) ? 1 : std::max<size_t>(i_set[s].count, 1);
        const size_t rr = (s + 1 == n_) ? 1 : std::max<size_t>(i_set[s + 1].count, 1);
        const size_t count = l * local_dims[s] * rr;
        if (count > stride) throw Error(T4A_GPU_BUFFER_TOO_SMALL, "import_site_shard: stride smaller than a site tensor");
        c.reshape(l, local_dims[s], rr);
        T4A_HIP(hipMemcpyAsync(c.buf.get(), d_src + (r * per_rank + s / shard_world) * stride, count * sizeof(double),
                               hipMemcpyDeviceToDevice, fill_.import_stream));
    }
    fill_.import_inflight = true;
}

} // namespace t4a
