// tt_canonical.hip — SiteTensorTrain / center_canonicalize, VidalTensorTrain and InverseTensorTrain on the device (see
// tt_canonical.hpp).  The sweeps are host-paced where the reference's bond dimension is data dependent (the rank of the rrLU, read
// back per site like TensorTrain::compress does); the Vidal right sweep knows its bonds in advance (min(L, S R), no truncation) and
// runs without a host turn of its own.  Every floating-point operation runs in the gfx950 kernels of kernels_rrlu*.hip,
// kernels_linalg.hip, kernels_dense.hip and kernels_tt.hip.  Cores are made, copied and read back with the helpers of tt_chain.hpp; the
// LU gauge steps stay here (they skip the reshape of the absorption helpers there and call the rrLU with their own options).
#include "tt_canonical.hpp"

#include <algorithm>

namespace t4a {

namespace {

void retire(GaugeScratch& w, DevCore& c) { w.retired.push_back(std::move(c.buf)); }

void settle(Engine& eng, GaugeScratch& w) // nothing in flight reads a retired buffer any more
{
    eng.sync();
    T4A_HIP(hipGetLastError());
    w.retired.clear();
}

// qr_decomp (canonical.rs:17-29): the rrLU that stops only at an exactly zero pivot, then left(true) / right(true) on the engine
size_t lu_for_qr(Engine& eng, const double* d_mat, int M, int N)
{
    if (M <= 0 || N <= 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "QR decomposition failed: empty bond matrix");
    const RrLUOptions o = RrLUOptions::from_abi((size_t)std::min(M, N), 0.0, 0.0, true);
    LuciResult r = eng.luci(d_mat, M, N, o, false, true);
    if (r.rank == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "QR decomposition failed: the bond matrix is zero (rank 0)");
    eng.lu_permuted_factors(r, true);
    return (size_t)r.rank;
}

// svd_factorize_right_matrix + the core updates of the Vidal right sweep (vidal.rs:309-361) at site i
void vidal_right_step(Engine& eng, std::vector<DevCore>& cores, size_t i, DevBuf<double>& sv, size_t& sv_len, GaugeScratch& w)
{
    hipStream_t st = eng.stream();
    DevCore& c = cores[i];
    DevCore& pv = cores[i - 1];
    const size_t L = c.l, S = c.s, R = c.r;
    if (L == 0 || S * R == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "Cannot compute Vidal singular values for an empty bond matrix");
    Engine::require_factor_dims(L, S * R, "Vidal bond SVD: dimensions");
    const size_t k = std::min(L, S * R);
    w.mat.reserve(c.size());
    w.u.reserve(L * k);
    w.vt.reserve(k * S * R);
    sv.reserve(k);
    core_reshape_launch(c.buf.get(), (int)L, (int)S, (int)R, 2, w.mat.get(), st);
    eng.svd(w.mat.get(), (int)L, (int)(S * R), w.u.get(), sv.get(), w.vt.get());
    sv_len = k;
    DevCore nc = DevCore::make(k, S, R); // V^T back in core layout
    core_reshape_launch(w.vt.get(), (int)k, (int)S, (int)R, 3, nc.buf.get(), st);
    // prev <- prev * (U diag(s)): prev in memory is already the (PL PS) x L matrix the product needs, and its output the new core
    w.fac.reserve(L * k);
    col_scale_launch(w.u.get(), (int)L, (int)L, (int)k, sv.get(), w.fac.get(), (int)L, st);
    const size_t PM = pv.l * pv.s;
    DevCore np = DevCore::make(pv.l, pv.s, k);
    if (PM) gemm_launch(gemm_desc((int)PM, (int)k, (int)L, pv.buf.get(), (int)PM, w.fac.get(), (int)L, np.buf.get(), (int)PM), st);
    retire(w, c);
    retire(w, pv);
    cores[i] = std::move(nc);
    cores[i - 1] = std::move(np);
}

// one launch of tt_bond_scale_kernel over `descs` (first_item and lanes are filled in here)
void bond_scale(Engine& eng, std::vector<TtScaleDesc>& descs, DevBuf<TtScaleDesc>& d_descs)
{
    std::vector<TtScaleDesc> live;
    unsigned long long items = 0;
    for (TtScaleDesc d : descs) {
        const unsigned long long n = tt_scale_items(d.l, d.s, d.r);
        if (n == 0) continue;
        d.lanes = tt_scale_lanes(d.l);
        d.first_item = items;
        items += n;
        live.push_back(d);
    }
    if (live.empty()) return;
    d_descs.reserve(live.size());
    T4A_HIP(hipMemcpyAsync(d_descs.get(), live.data(), live.size() * sizeof(TtScaleDesc), hipMemcpyHostToDevice, eng.stream()));
    tt_bond_scale_launch(d_descs.get(), (int)live.size(), items, eng.stream());
    T4A_HIP(hipGetLastError());
    eng.sync(); // `live` is pageable host memory
}

TtScaleDesc scale_desc(const double* src, double* dst, size_t l, size_t s, size_t r)
{
    TtScaleDesc d{};
    d.src = src;
    d.dst = dst;
    d.l = (int)l;
    d.s = (int)s;
    d.r = (int)r;
    d.lop = d.rop = TT_SCALE_NONE;
    return d;
}

void check_core_dims(const size_t d[3])
{
    if (d[0] > 65535 || d[1] > 65535 || d[2] > 65535)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "tensor train dimensions above 65535 are not supported");
}

// to_tensor_train of the Vidal and the inverse form: every core but the last times its right-bond vector
std::vector<DevCore> times_right_vectors(Engine& eng, const std::vector<DevCore>& cores, const std::vector<DevBuf<double>>& vec,
                                         const std::vector<size_t>& len)
{
    const size_t n = cores.size();
    std::vector<DevCore> out(n);
    std::vector<TtScaleDesc> descs;
    for (size_t i = 0; i < n; ++i) {
        out[i] = DevCore::make(cores[i].l, cores[i].s, cores[i].r);
        TtScaleDesc d = scale_desc(cores[i].buf.get(), out[i].buf.get(), cores[i].l, cores[i].s, cores[i].r);
        if (i + 1 < n) {
            d.rop = TT_SCALE_MUL;
            d.rv = vec[i].get();
            d.rn = (int)len[i];
        }
        descs.push_back(d);
    }
    DevBuf<TtScaleDesc> table;
    bond_scale(eng, descs, table);
    return out;
}

void upload_vector(Engine& eng, DevBuf<double>& dst, const double* host, size_t len)
{
    dst.reserve(std::max<size_t>(len, 1));
    if (len) {
        T4A_HIP(hipMemcpyAsync(dst.get(), host, len * sizeof(double), hipMemcpyHostToDevice, eng.stream()));
        eng.sync();
    }
}

std::string two_site_message(size_t i, size_t n) // canonical.rs:379-387, vidal.rs:713-721 (len() - 2 wraps there for n < 2)
{
    return "Cannot set two-site tensors at site " + std::to_string(i) + " (max " + std::to_string(n - 2) + ")";
}

} // namespace

void replace_core(Engine& eng, DevCore& dst, const size_t dims[3], const double* host, GaugeScratch& w)
{
    check_core_dims(dims);
    DevCore c = DevCore::make(dims[0], dims[1], dims[2]);
    if (c.size()) {
        if (!host) throw Error(T4A_GPU_NULL_POINTER, "tensor data is null");
        T4A_HIP(hipMemcpyAsync(c.buf.get(), host, c.size() * sizeof(double), hipMemcpyHostToDevice, eng.stream()));
    }
    retire(w, dst);
    dst = std::move(c);
    settle(eng, w);
}

void gauge_left_step(Engine& eng, std::vector<DevCore>& cores, size_t i, GaugeScratch& w)
{
    if (i + 1 >= cores.size()) return; // canonical.rs:192-194
    hipStream_t st = eng.stream();
    DevCore& c = cores[i];
    DevCore& nx = cores[i + 1];
    const int L = (int)c.l, S = (int)c.s, R = (int)c.r;
    w.mat.reserve(std::max<size_t>(c.size(), 1));
    core_reshape_launch(c.buf.get(), L, S, R, 0, w.mat.get(), st); // rows l * S + s (canonical.rs:39-55)
    const size_t rk = lu_for_qr(eng, w.mat.get(), L * S, R);
    DevCore nc = DevCore::make(c.l, c.s, rk);
    core_reshape_launch(eng.left(), L, S, (int)rk, 1, nc.buf.get(), st);
    // next <- right(true) (rk x R) * next: a core in memory is the column-major R x (S' R') matrix and the product's output the new core
    // (the reference's column order s * R' + r of tensor3_to_right_matrix only permutes the columns of both sides of the product)
    const size_t cols = nx.s * nx.r;
    DevCore nn = DevCore::make(rk, nx.s, nx.r);
    if (cols) gemm_launch(gemm_desc((int)rk, (int)cols, R, eng.right(), (int)rk, nx.buf.get(), R, nn.buf.get(), (int)rk), st);
    retire(w, c);
    retire(w, nx);
    cores[i] = std::move(nc);
    cores[i + 1] = std::move(nn);
    settle(eng, w); // the engine's factor buffers are reused by the next step
}

void gauge_right_step(Engine& eng, std::vector<DevCore>& cores, size_t i, GaugeScratch& w)
{
    if (i == 0) return; // canonical.rs:245-247
    hipStream_t st = eng.stream();
    DevCore& c = cores[i];
    DevCore& pv = cores[i - 1];
    const size_t L = c.l, S = c.s, R = c.r;
    // transpose(tensor3_to_right_matrix): (S R) x L with row s * R + r — the axis reversal (l, s, r) -> (r, s, l) of the core
    w.mat.reserve(std::max<size_t>(c.size(), 1));
    {
        const size_t dims[3] = {L, S, R}, perm[3] = {2, 1, 0};
        permute_launch(c.buf.get(), dims, perm, 3, w.mat.get(), st);
    }
    const size_t rk = lu_for_qr(eng, w.mat.get(), (int)(S * R), (int)L);
    // Q = left(true)^T: the (R, S, rk) block reversed to (rk, S, R) is the new core
    DevCore nc = DevCore::make(rk, S, R);
    {
        const size_t dims[3] = {R, S, rk}, perm[3] = {2, 1, 0};
        permute_launch(eng.left(), dims, perm, 3, nc.buf.get(), st);
    }
    // prev <- prev (PL PS x L) * right(true)^T (L x rk), again in core layout on both sides
    const size_t PM = pv.l * pv.s;
    DevCore np = DevCore::make(pv.l, pv.s, rk);
    if (PM) {
        GemmDesc g = gemm_desc((int)PM, (int)rk, (int)L, pv.buf.get(), (int)PM, eng.right(), (int)rk, np.buf.get(), (int)PM);
        g.transB = 1;
        gemm_launch(g, st);
    }
    retire(w, c);
    retire(w, pv);
    cores[i] = std::move(nc);
    cores[i - 1] = std::move(np);
    settle(eng, w);
}

void center_canonicalize(TensorTrain& tt, size_t center)
{
    const size_t n = tt.cores.size();
    if (n <= 1 || center >= n) return; // canonical.rs:443-446
    GaugeScratch w;
    for (size_t i = 0; i < center; ++i) gauge_left_step(tt.eng, tt.cores, i, w);
    for (size_t i = n - 1; i > center; --i) gauge_right_step(tt.eng, tt.cores, i, w);
}

// ------------------------------------------------------------------------------------------------
// SiteTensorTrain (canonical.rs:118-393)
// ------------------------------------------------------------------------------------------------
void SiteTrain::check_new(size_t n, size_t center)
{
    if (n == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "Tensor train is empty");
    if (center >= n)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Center " + std::to_string(center) + " is out of range for " + std::to_string(n) + " tensors");
}

SiteTrain::SiteTrain(const std::vector<DevCore>& src, hipStream_t src_stream, size_t center) : center_(center)
{
    check_new(src.size(), center);
    for (size_t i = 0; i + 1 < src.size(); ++i)
        if (src[i].r != src[i + 1].l)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Dimension mismatch: tensor at site " + std::to_string(i) + " has incompatible dimensions");
    if (src_stream) T4A_HIP(hipStreamSynchronize(src_stream));
    cores = clone_cores(src, eng.stream());
    const size_t n = cores.size();
    if (n > 1) { // canonicalize (canonical.rs:172-188)
        for (size_t i = 0; i < center_; ++i) gauge_left_step(eng, cores, i, w_);
        for (size_t i = n - 1; i > center_; --i) gauge_right_step(eng, cores, i, w_);
    }
    settle(eng, w_);
}

void SiteTrain::move_center_right()
{
    if (center_ + 1 >= len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "Cannot move center right: already at rightmost position");
    gauge_left_step(eng, cores, center_, w_);
    ++center_;
}

void SiteTrain::move_center_left()
{
    if (center_ == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "Cannot move center left: already at leftmost position");
    gauge_right_step(eng, cores, center_, w_);
    --center_;
}

void SiteTrain::set_center(size_t new_center)
{
    if (new_center >= len())
        throw Error(T4A_GPU_INVALID_ARGUMENT,
                    "New center " + std::to_string(new_center) + " is out of range for " + std::to_string(len()) + " tensors");
    while (center_ < new_center) move_center_right();
    while (center_ > new_center) move_center_left();
}

void SiteTrain::set_site_tensor(size_t i, const size_t dims[3], const double* host)
{
    if (i >= len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "site " + std::to_string(i) + " is out of range for " + std::to_string(len()) + " tensors");
    replace_core(eng, cores[i], dims, host, w_);
}

void SiteTrain::set_two_site_tensors(size_t i, const size_t d1[3], const double* t1, const size_t d2[3], const double* t2)
{
    if (len() < 2 || i >= len() - 1) throw Error(T4A_GPU_INVALID_ARGUMENT, two_site_message(i, len()));
    check_core_dims(d1);
    check_core_dims(d2);
    if ((d1[0] * d1[1] * d1[2] && !t1) || (d2[0] * d2[1] * d2[2] && !t2)) throw Error(T4A_GPU_NULL_POINTER, "tensor data is null");
    replace_core(eng, cores[i], d1, t1, w_);
    replace_core(eng, cores[i + 1], d2, t2, w_);
}

// ------------------------------------------------------------------------------------------------
// VidalTensorTrain (vidal.rs:215-493)
// ------------------------------------------------------------------------------------------------
void VidalTrain::check_partition(size_t n, size_t end)
{
    if (n != 0 && end > n)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Partition end " + std::to_string(end) + " exceeds tensor train length " + std::to_string(n));
}

void VidalTrain::check_new(size_t n, size_t n_svs)
{
    if (n != 0 && n_svs != n - 1)
        throw Error(T4A_GPU_INVALID_ARGUMENT, "Expected " + std::to_string(n - 1) + " singular value vectors, got " + std::to_string(n_svs));
}

VidalTrain::VidalTrain(const std::vector<DevCore>& src, hipStream_t src_stream, size_t start, size_t end)
{
    const size_t n = src.size();
    if (n == 0) return; // vidal.rs:238-244: the empty object, partition 0..0
    check_partition(n, end);
    eng = std::make_unique<Engine>();
    if (src_stream) T4A_HIP(hipStreamSynchronize(src_stream));
    cores = clone_cores(src, eng->stream());
    sv.resize(n - 1);
    sv_len.assign(n - 1, 0);
    part_start = start;
    part_end = end;
    if (start >= end) { // an empty range: nothing is re-gauged
        settle(*eng, w_);
        return;
    }
    // left sweep (vidal.rs:259-306): the LU-for-QR step of the site form
    for (size_t i = start; i + 1 < end; ++i) gauge_left_step(*eng, cores, i, w_);
    // right sweep (vidal.rs:309-361): the bond is min(L, S R), known in advance — no host turn besides those of Engine::svd
    for (size_t i = end; i-- > start + 1;) vidal_right_step(*eng, cores, i, sv[i - 1], sv_len[i - 1], w_);
    // division pass (vidal.rs:364-388), one launch, in place
    std::vector<TtScaleDesc> descs;
    for (size_t i = start; i + 1 < end; ++i) {
        if (sv_len[i] == 0) continue;
        TtScaleDesc d = scale_desc(cores[i].buf.get(), cores[i].buf.get(), cores[i].l, cores[i].s, cores[i].r);
        d.rop = TT_SCALE_DIV_GUARD;
        d.rv = sv[i].get();
        d.rn = (int)sv_len[i];
        descs.push_back(d);
    }
    DevBuf<TtScaleDesc> table;
    bond_scale(*eng, descs, table);
    settle(*eng, w_);
}

VidalTrain::VidalTrain(const std::vector<std::array<size_t, 3>>& dims3, const double* cores_host, const std::vector<size_t>& sv_lens,
                       const double* svs_host)
{
    const size_t n = dims3.size();
    if (n == 0) return;
    check_new(n, sv_lens.size());
    size_t total = 0, sv_total = 0;
    for (const auto& d : dims3) {
        check_core_dims(d.data());
        total += d[0] * d[1] * d[2];
    }
    for (size_t k : sv_lens) sv_total += k;
    if (total && !cores_host) throw Error(T4A_GPU_NULL_POINTER, "core data is null");
    if (sv_total && !svs_host) throw Error(T4A_GPU_NULL_POINTER, "singular value data is null");
    require_device();
    eng = std::make_unique<Engine>();
    cores.resize(n);
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) {
        cores[i] = DevCore::make(dims3[i][0], dims3[i][1], dims3[i][2]);
        if (cores[i].size())
            T4A_HIP(hipMemcpyAsync(cores[i].buf.get(), cores_host + off, cores[i].size() * sizeof(double), hipMemcpyHostToDevice, eng->stream()));
        off += cores[i].size();
    }
    sv.resize(n - 1);
    sv_len = sv_lens;
    off = 0;
    for (size_t b = 0; b + 1 < n; ++b) {
        sv[b].reserve(std::max<size_t>(sv_len[b], 1));
        if (sv_len[b])
            T4A_HIP(hipMemcpyAsync(sv[b].get(), svs_host + off, sv_len[b] * sizeof(double), hipMemcpyHostToDevice, eng->stream()));
        off += sv_len[b];
    }
    part_start = 0;
    part_end = n;
    eng->sync();
}

std::vector<double> VidalTrain::singular_values_host(size_t bond)
{
    if (bond >= sv.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "bond " + std::to_string(bond) + " is out of range for " + std::to_string(sv.size()) + " singular value vectors");
    return to_host(*eng, sv[bond].get(), sv_len[bond]);
}

void VidalTrain::set_singular_values(size_t bond, const double* host, size_t len)
{
    if (bond >= sv.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "bond " + std::to_string(bond) + " is out of range for " + std::to_string(sv.size()) + " singular value vectors");
    if (len && !host) throw Error(T4A_GPU_NULL_POINTER, "singular value data is null");
    eng->sync();
    upload_vector(*eng, sv[bond], host, len);
    sv_len[bond] = len;
}

void VidalTrain::set_site_tensor(size_t i, const size_t dims[3], const double* host)
{
    if (i >= len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "site " + std::to_string(i) + " is out of range for " + std::to_string(len()) + " tensors");
    replace_core(*eng, cores[i], dims, host, w_);
}

std::vector<DevCore> VidalTrain::to_tensor_train_cores()
{
    if (cores.empty()) return {};
    return times_right_vectors(*eng, cores, sv, sv_len);
}

// ------------------------------------------------------------------------------------------------
// InverseTensorTrain (vidal.rs:551-767)
// ------------------------------------------------------------------------------------------------
InverseTrain::InverseTrain(VidalTrain& vidal)
{
    const size_t n = vidal.len();
    part_start = vidal.part_start;
    part_end = vidal.part_end;
    if (n == 0) return;
    eng = std::make_unique<Engine>();
    vidal.eng->sync();
    cores.resize(n);
    inv.resize(n - 1);
    inv_len = vidal.sv_len;
    std::vector<TtScaleDesc> descs;
    // first core: right factor only; middle cores: (val * sv[i-1][l]) * sv[i][r]; last core: left factor only (vidal.rs:563-645)
    for (size_t i = 0; i < n; ++i) {
        const DevCore& c = vidal.cores[i];
        cores[i] = DevCore::make(c.l, c.s, c.r);
        TtScaleDesc d = scale_desc(c.buf.get(), cores[i].buf.get(), c.l, c.s, c.r);
        if (i > 0) {
            d.lop = TT_SCALE_MUL;
            d.lv = vidal.sv[i - 1].get();
            d.ln = (int)vidal.sv_len[i - 1];
        }
        if (i + 1 < n) {
            d.rop = TT_SCALE_MUL;
            d.rv = vidal.sv[i].get();
            d.rn = (int)vidal.sv_len[i];
        }
        descs.push_back(d);
    }
    // inverse values (vidal.rs:648-656): the vector as a (len, 1, 1) block
    for (size_t b = 0; b + 1 < n; ++b) {
        inv[b].reserve(std::max<size_t>(inv_len[b], 1));
        TtScaleDesc d = scale_desc(vidal.sv[b].get(), inv[b].get(), inv_len[b], 1, 1);
        d.lop = TT_SCALE_INVERT;
        descs.push_back(d);
    }
    DevBuf<TtScaleDesc> table;
    bond_scale(*eng, descs, table);
    settle(*eng, w_);
}

std::vector<double> InverseTrain::inverse_singular_values_host(size_t bond)
{
    if (bond >= inv.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "bond " + std::to_string(bond) + " is out of range for " + std::to_string(inv.size()) + " singular value vectors");
    return to_host(*eng, inv[bond].get(), inv_len[bond]);
}

void InverseTrain::set_two_site_tensors(size_t i, const size_t d1[3], const double* t1, const double* inv_sv, size_t n_inv, const size_t d2[3],
                                        const double* t2)
{
    if (len() < 2 || i >= len() - 1) throw Error(T4A_GPU_INVALID_ARGUMENT, two_site_message(i, len()));
    check_core_dims(d1);
    check_core_dims(d2);
    if (n_inv && !inv_sv) throw Error(T4A_GPU_NULL_POINTER, "inverse singular value data is null");
    if ((d1[0] * d1[1] * d1[2] && !t1) || (d2[0] * d2[1] * d2[2] && !t2)) throw Error(T4A_GPU_NULL_POINTER, "tensor data is null");
    replace_core(*eng, cores[i], d1, t1, w_);
    upload_vector(*eng, inv[i], inv_sv, n_inv);
    inv_len[i] = n_inv;
    replace_core(*eng, cores[i + 1], d2, t2, w_);
}

std::vector<DevCore> InverseTrain::to_tensor_train_cores()
{
    if (cores.empty()) return {};
    return times_right_vectors(*eng, cores, inv, inv_len);
}

} // namespace t4a
