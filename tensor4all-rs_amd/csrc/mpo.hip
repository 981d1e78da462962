// mpo.hip — MPO<f64> and the contraction of two MPOs on the device (see mpo.hpp).  Shape bookkeeping is host work; every
// floating-point operation runs in gfx950 kernels: the naive site contraction (kernels_mpo.hip), the f64-MFMA GEMM and the
// gathers (kernels_dense.hip), the axis permutation (kernels_tt.hip), the Householder QR and the Jacobi SVD (kernels_linalg.hip),
// the half products of the variational fit (kernels_mpo_fit.hip), the site and half products of the partial contraction
// (kernels_partial.hip; the host plan mpo_partial_plan is at the end of this file).  Sites are made, copied, right-canonicalised (QrSweep) and split
// after the two-site SVD (split_two_site) with the chain helpers of tt_chain.hpp.
#include "mpo.hpp"
#include "linop.hpp"
#include "krylov.hpp"
#include "tensorops.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>

namespace t4a {

namespace {

constexpr size_t MPO_DIM_MAX = 65535; // the tensor train's limit, which also holds for the fused site index s1*s2

// the kernels and the GEMM index a site with int
void check_count(size_t a, size_t b, size_t c, size_t d, const std::string& what)
{
    const unsigned long long lim = INT_MAX;
    unsigned long long n = 1;
    for (size_t x : {a, b, c, d}) {
        if (x > lim || n * x > lim) throw Error(T4A_GPU_INVALID_ARGUMENT, what + " holds more than INT_MAX elements");
        n *= x;
    }
}

// One contraction: every launch goes to the stream of `eng` (the engine of the left operand).
struct Contractor {
    Engine& eng;
    const MpoContractionOptions& opt;
    hipStream_t st;
    DevBuf<double> u, s, vt, m1, m2, x, y, cm;
    std::vector<double> hs;
    QrSweep sweeper; // right_canonicalize (canonical.rs:35-89) is sweeper.canonicalize(cores, 0)

    // the site plans of a partial contraction (mpo_partial_contract*); null: the matrix product, on the code path it always had
    const std::vector<PartialSitePlan>* plan = nullptr;
    // the site kinds of an operator applied on a subset of the state's sites (linop.hpp: linop_fused_contract); null everywhere else.
    // At a gap site `a` holds a shape only (the pass-through bond) and the half product is that of kernels_apply.hip.
    const std::vector<ApplySitePlan>* gaps = nullptr;

    Contractor(Engine& e, const MpoContractionOptions& o) : eng(e), opt(o), st(e.stream()), sweeper(e) {}

    // the fused site dimension s * t of the product at site i
    size_t st_dim(const Mpo& a, const Mpo& b, size_t i) const { return plan ? (*plan)[i].S * (*plan)[i].T : a.sd[i][0] * b.sd[i][1]; }

    // factorize (factorize.rs:126-313) with left_orthogonal = true, SVD rank rule: cutoff = tolerance * s_max, values kept
    // while rank < max_bond_dim and s >= cutoff; a zero matrix keeps nothing and is floored to rank 1 (not an error).  LU and
    // CI fall back to SVD (:133-137).  U (M x k), S (k), Vt (k x N) stay in u / s / vt for left() / right().
    size_t svd_rank(const double* d_mat, int M, int N)
    {
        if (opt.method == MpoFactorizeMethod::RSVD)
            throw Error(T4A_GPU_NOT_IMPLEMENTED, "Factorization failed: RSVD factorization not yet implemented"); // :305-313
        const int k = std::min(M, N);
        u.reserve((size_t)M * k);
        s.reserve(k);
        vt.reserve((size_t)k * N);
        eng.svd(d_mat, M, N, u.get(), s.get(), vt.get());
        hs.resize(k);
        T4A_HIP(hipMemcpyAsync(hs.data(), s.get(), sizeof(double) * k, hipMemcpyDeviceToHost, st));
        eng.sync();
        double s_max = 0.0;
        for (double v : hs) s_max = std::max(s_max, v);
        size_t rank = 0;
        if (s_max > 0.0) {
            const double cutoff = opt.tolerance * s_max;
            for (int i = 0; i < k; ++i) {
                if (opt.max_bond_dim != 0 && rank >= opt.max_bond_dim) break;
                if (hs[i] < cutoff) break;
                ++rank;
            }
        }
        return std::max<size_t>(rank, 1);
    }
    // left = U[:, :rank] (M x rank)
    void left(int M, int rank, double* out) { gather_launch(u.get(), M, nullptr, M, nullptr, rank, out, M, st); }
    // right = diag(S[:rank]) Vt[:rank, :] (rank x N)
    void right(int M, int N, int rank, double* out) { diag_scale_launch(vt.get(), std::min(M, N), rank, N, s.get(), true, out, rank, st); }

    // contract_site_tensors (environment.rs:37-80) of every site in one launch
    std::vector<DevCore> naive(const Mpo& a, const Mpo& b)
    {
        const size_t n = a.len();
        std::vector<DevCore> out(n);
        std::vector<MpoSiteJob> jobs(n);
        unsigned long long off = 0;
        for (size_t i = 0; i < n; ++i) {
            const DevCore& x = a.tt.cores[i];
            const DevCore& y = b.tt.cores[i];
            const size_t s1 = a.sd[i][0], k = a.sd[i][1], t = b.sd[i][1];
            check_count(x.l * y.l, s1, t, x.r * y.r, "contract_naive: site " + std::to_string(i));
            out[i] = DevCore::make(x.l * y.l, s1 * t, x.r * y.r);
            MpoSiteJob& j = jobs[i];
            j = MpoSiteJob{};
            j.A = x.buf.get();
            j.B = y.buf.get();
            j.C = out[i].buf.get();
            j.off = off;
            j.la = (int)x.l;
            j.s1 = (int)s1;
            j.k = (int)k;
            j.ra = (int)x.r;
            j.lb = (int)y.l;
            j.t = (int)t;
            j.rb = (int)y.r;
            off += out[i].size();
        }
        DevBuf<MpoSiteJob> d_jobs;
        d_jobs.reserve(n);
        T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), n * sizeof(MpoSiteJob), hipMemcpyHostToDevice, st));
        mpo_site_contract_launch(d_jobs.get(), (int)n, off, st);
        T4A_HIP(hipGetLastError());
        eng.sync(); // `jobs` is pageable host memory, d_jobs goes out of scope
        return out;
    }

    // the site product of a plan for every site in one launch (kernels_partial.hip)
    std::vector<DevCore> naive_partial(const Mpo& a, const Mpo& b)
    {
        const size_t n = a.len();
        std::vector<DevCore> out(n);
        std::vector<MpoPartialSiteJob> jobs(n);
        unsigned long long off = 0;
        for (size_t i = 0; i < n; ++i) {
            const DevCore& x = a.tt.cores[i];
            const DevCore& y = b.tt.cores[i];
            const PartialSitePlan& p = (*plan)[i];
            check_count(x.l * y.l, p.S, p.T, x.r * y.r, "partial_contract: site " + std::to_string(i));
            out[i] = DevCore::make(x.l * y.l, p.S * p.T, x.r * y.r);
            MpoPartialSiteJob& j = jobs[i];
            j = MpoPartialSiteJob{};
            j.A = x.buf.get();
            j.B = y.buf.get();
            j.C = out[i].buf.get();
            j.off = off;
            j.la = (int)x.l, j.FA = (int)x.s, j.ra = (int)x.r;
            j.lb = (int)y.l, j.FB = (int)y.s, j.rb = (int)y.r;
            j.S = (int)p.S, j.K = (int)p.K, j.T = (int)p.T;
            j.s0 = (int)p.s0, j.k0 = (int)p.k0, j.t0 = (int)p.t0;
            j.as0 = (int)p.as[0], j.as1 = (int)p.as[1], j.ak0 = (int)p.ak[0], j.ak1 = (int)p.ak[1];
            j.bs0 = (int)p.bs[0], j.bs1 = (int)p.bs[1], j.bk0 = (int)p.bk[0], j.bk1 = (int)p.bk[1];
            j.bt0 = (int)p.bt[0], j.bt1 = (int)p.bt[1];
            off += out[i].size();
        }
        DevBuf<MpoPartialSiteJob> d_jobs;
        d_jobs.reserve(n);
        T4A_HIP(hipMemcpyAsync(d_jobs.get(), jobs.data(), n * sizeof(MpoPartialSiteJob), hipMemcpyHostToDevice, st));
        mpo_partial_site_launch(d_jobs.get(), (int)n, off, st);
        T4A_HIP(hipGetLastError());
        eng.sync(); // `jobs` is pageable host memory, d_jobs goes out of scope
        return out;
    }

    // compress_mpo (contract_naive.rs:100-172): right-canonicalise, then a left-to-right sweep of factorize; the right factor
    // is absorbed into the next site
    void compress(std::vector<DevCore>& cores)
    {
        const size_t n = cores.size();
        if (n <= 1) return;
        sweeper.canonicalize(cores, 0);
        for (size_t i = 0; i + 1 < n; ++i) {
            DevCore& c = cores[i];
            DevCore& nx = cores[i + 1];
            const int M = (int)(c.l * c.s), N = (int)c.r;
            const size_t rank = svd_rank(c.buf.get(), M, N);
            DevCore nc = DevCore::make(c.l, c.s, rank);
            left(M, (int)rank, nc.buf.get());
            m2.reserve(rank * N);
            right(M, N, (int)rank, m2.get());
            DevCore nn = DevCore::make(rank, nx.s, nx.r);
            const int rest = (int)(nx.s * nx.r);
            gemm_launch(gemm_desc((int)rank, rest, N, m2.get(), (int)rank, nx.buf.get(), N, nn.buf.get(), (int)rank), st);
            T4A_HIP(hipGetLastError());
            eng.sync();
            c = std::move(nc);
            nx = std::move(nn);
        }
    }

    // contract_zipup (contract_zipup.rs:45-167).  Per site two pairwise contractions on the MFMA GEMM (never the three-operand
    // sum, :118-127) and one permutation of the large intermediate; the small input site tensors are permuted so that both
    // contracted index pairs come out adjacent:
    //   A'[a, s, c, k] = A[a, s, k, c]                    B'[k, b, t, d] = B[b, k, t, d]
    //   X[n, s, c, k, b] = sum_a R[n, a, b] A'[a, s, c, k]  (one GEMM per b)
    //   Y[n, s, c, t, d] = sum_{k, b} X[(n, s, c), (k, b)] B'[(k, b), (t, d)]
    //   C[n, s, t, c, d] = Y permuted, factorised as (n*s*t) x (c*d): left -> site, right -> the next remainder R[rank, c, d]
    std::vector<DevCore> zipup(const Mpo& a, const Mpo& b)
    {
        const size_t n = a.len();
        std::vector<DevCore> out;
        DevBuf<double> rem, rem_next;
        rem.reserve(1);
        fill_launch(rem.get(), 1, 1.0, st); // R[new, a, b] = [[[1]]]
        size_t N0 = 1;
        for (size_t i = 0; i < n; ++i) {
            const DevCore& A = a.tt.cores[i];
            const DevCore& B = b.tt.cores[i];
            const size_t La = A.l, S1 = a.sd[i][0], K = a.sd[i][1], Ra = A.r;
            const size_t Lb = B.l, T = b.sd[i][1], Rb = B.r;
            const std::string where = "contract_zipup: site " + std::to_string(i);
            check_count(N0 * S1, Ra, K, Lb, where);
            check_count(N0 * S1, Ra, T, Rb, where);
            m1.reserve(A.size());
            m2.reserve(B.size());
            const size_t da[4] = {La, S1, K, Ra}, pa[4] = {0, 1, 3, 2};
            const size_t db[4] = {Lb, K, T, Rb}, pb[4] = {1, 0, 2, 3};
            permute_launch(A.buf.get(), da, pa, 4, m1.get(), st);
            permute_launch(B.buf.get(), db, pb, 4, m2.get(), st);
            const size_t xcols = S1 * Ra * K;
            x.reserve(N0 * xcols * Lb);
            GemmDesc g = gemm_desc((int)N0, (int)xcols, (int)La, rem.get(), (int)N0, m1.get(), (int)La, x.get(), (int)N0);
            g.strideA = (long long)(N0 * La);
            g.strideB = 0;
            g.strideC = (long long)(N0 * xcols);
            g.batch = (int)Lb;
            gemm_launch(g, st);
            const size_t rows = N0 * S1 * Ra, cols = T * Rb;
            if (i == n - 1) { // last site: the trailing bonds are 1, Y is C = [n, s1, t, 1]
                DevCore site = DevCore::make(N0, S1 * T, 1);
                gemm_launch(gemm_desc((int)rows, (int)cols, (int)(K * Lb), x.get(), (int)rows, m2.get(), (int)(K * Lb), site.buf.get(), (int)rows),
                            st);
                T4A_HIP(hipGetLastError());
                eng.sync();
                out.push_back(std::move(site));
                break;
            }
            y.reserve(rows * cols);
            gemm_launch(gemm_desc((int)rows, (int)cols, (int)(K * Lb), x.get(), (int)rows, m2.get(), (int)(K * Lb), y.get(), (int)rows), st);
            const size_t dy[5] = {N0, S1, Ra, T, Rb}, py[5] = {0, 1, 3, 2, 4};
            cm.reserve(rows * cols);
            permute_launch(y.get(), dy, py, 5, cm.get(), st);
            const int M = (int)(N0 * S1 * T), N = (int)(Ra * Rb);
            const size_t rank = svd_rank(cm.get(), M, N);
            DevCore site = DevCore::make(N0, S1 * T, rank);
            left(M, (int)rank, site.buf.get());
            rem_next.reserve(rank * N);
            right(M, N, (int)rank, rem_next.get());
            T4A_HIP(hipGetLastError());
            eng.sync();
            std::swap(rem, rem_next);
            N0 = rank;
            out.push_back(std::move(site));
        }
        return out;
    }

    // zipup for a plan: the site step C[n, s, t, c, d] = R A_i B_i is ONE launch of the half product with E = the remainder, and its
    // output is the (n s t) x (c d) matrix svd_rank reads: no permutation of a site or of the intermediate.  left() / right() and the
    // last-site rule are those of zipup.
    std::vector<DevCore> zipup_partial(const Mpo& a, const Mpo& b)
    {
        const size_t n = a.len();
        std::vector<DevCore> out;
        DevBuf<double> rem, rem_next;
        rem.reserve(1);
        fill_launch(rem.get(), 1, 1.0, st); // R[new, a, b] = [[[1]]]
        size_t N0 = 1;
        for (size_t i = 0; i < n; ++i) {
            const size_t Ra = a.tt.cores[i].r, Rb = b.tt.cores[i].r, ST = st_dim(a, b, i);
            if (i == n - 1) { // last site: the trailing bonds are 1, the half product is C = [n, s t, 1]
                DevCore site = DevCore::make(N0, ST, 1);
                half_into(a, b, i, false, rem.get(), N0, site.buf.get(), "partial_contract (zipup): site ");
                T4A_HIP(hipGetLastError());
                eng.sync();
                out.push_back(std::move(site));
                break;
            }
            half(a, b, i, false, rem.get(), N0, cm, "partial_contract (zipup): site ");
            const int M = (int)(N0 * ST), N = (int)(Ra * Rb);
            const size_t rank = svd_rank(cm.get(), M, N);
            DevCore site = DevCore::make(N0, ST, rank);
            left(M, (int)rank, site.buf.get());
            rem_next.reserve(rank * N);
            right(M, N, (int)rank, rem_next.get());
            T4A_HIP(hipGetLastError());
            eng.sync();
            std::swap(rem, rem_next);
            N0 = rank;
            out.push_back(std::move(site));
        }
        return out;
    }

    // ---- variational fit (mpo.hpp: mpo_contract_fit).  C_i[c_i, s, t, c_{i+1}] is the fitted MPO,
    //   L_i[c_i, la_i, lb_i] the contraction of the sites < i of A, B and C,  R_i[la_i, lb_i, c_i] that of the sites >= i,
    //   P_i[c_i, s, t, la', lb'] = L_i A_i B_i   and   Q_i[la, lb, s, t, c_{i+1}] = A_i B_i R_{i+1}   the half products,
    // all column-major, so that P_i is a (c_i s t) x (la' lb') matrix and Q_i a (la lb) x (s t c_{i+1}) matrix as they stand.
    std::vector<DevBuf<double>> envL, envR; // envL[i] = L_i (i < n), envR[i] = R_i (1 <= i <= n)
    DevBuf<double> hp, hq, theta;

    static MpoFitHalfDesc half_desc(bool right, const double* env, size_t n_env, const double* A, size_t la, size_t s, size_t k, size_t ra,
                                    const double* B, size_t lb, size_t t, size_t rb, double* out)
    {
        MpoFitHalfDesc d{};
        d.E = env;
        d.A = A;
        d.B = B;
        d.out = out;
        d.N = (int)n_env;
        d.S = (int)s;
        d.K = (int)k;
        d.T = (int)t;
        // A[la, s, k, ra], B[lb, k, t, rb]
        d.as = (long long)la;
        d.ak = (long long)(la * s);
        d.bk = (long long)lb;
        d.bt = (long long)(lb * k);
        const long long a_l = 1, a_r = (long long)(la * s * k), b_l = 1, b_r = (long long)(lb * k * t);
        if (!right) { // P: E = L[n, la, lb], out[n, s, t, ra, rb]
            d.La = (int)la, d.Lb = (int)lb, d.C = (int)ra, d.D = (int)rb;
            d.en = 1, d.ea = (long long)n_env, d.eb = (long long)(n_env * la);
            d.aa = a_l, d.ac = a_r, d.bb = b_l, d.bd = b_r;
            d.on = 1, d.os = (long long)n_env, d.ot = (long long)(n_env * s), d.oc = (long long)(n_env * s * t),
            d.od = (long long)(n_env * s * t * ra);
        } else { // Q: E = R[ra, rb, n], out[la, lb, s, t, n]
            d.La = (int)ra, d.Lb = (int)rb, d.C = (int)la, d.D = (int)lb;
            d.ea = 1, d.eb = (long long)ra, d.en = (long long)(ra * rb);
            d.aa = a_r, d.ac = a_l, d.bb = b_r, d.bd = b_l;
            d.oc = 1, d.od = (long long)la, d.os = (long long)(la * lb), d.ot = (long long)(la * lb * s), d.on = (long long)(la * lb * s * t);
        }
        return d;
    }

    // half_desc for a site plan: the strides of s, kappa and t per leg, and those of B along s (a diagonal pair)
    static MpoPartialHalfDesc partial_half_desc(bool right, const double* env, size_t n_env, const DevCore& A, const DevCore& B,
                                                const PartialSitePlan& p, double* out)
    {
        MpoPartialHalfDesc d{};
        const size_t la = A.l, ra = A.r, lb = B.l, rb = B.r, s = p.S, t = p.T;
        d.E = env;
        d.A = A.buf.get();
        d.B = B.buf.get();
        d.out = out;
        d.N = (int)n_env;
        d.S = (int)s, d.K = (int)p.K, d.T = (int)t;
        d.s0 = (int)p.s0, d.k0 = (int)p.k0, d.t0 = (int)p.t0;
        // A[la, fA, ra], B[lb, fB, rb]
        d.as0 = (long long)(la * p.as[0]), d.as1 = (long long)(la * p.as[1]);
        d.ak0 = (long long)(la * p.ak[0]), d.ak1 = (long long)(la * p.ak[1]);
        d.bs0 = (long long)(lb * p.bs[0]), d.bs1 = (long long)(lb * p.bs[1]);
        d.bk0 = (long long)(lb * p.bk[0]), d.bk1 = (long long)(lb * p.bk[1]);
        d.bt0 = (long long)(lb * p.bt[0]), d.bt1 = (long long)(lb * p.bt[1]);
        const long long a_l = 1, a_r = (long long)(la * A.s), b_l = 1, b_r = (long long)(lb * B.s);
        if (!right) { // P: E = L[n, la, lb], out[n, s, t, ra, rb]
            d.La = (int)la, d.Lb = (int)lb, d.C = (int)ra, d.D = (int)rb;
            d.en = 1, d.ea = (long long)n_env, d.eb = (long long)(n_env * la);
            d.aa = a_l, d.ac = a_r, d.bb = b_l, d.bd = b_r;
            d.on = 1, d.os = (long long)n_env, d.ot = (long long)(n_env * s), d.oc = (long long)(n_env * s * t),
            d.od = (long long)(n_env * s * t * ra);
        } else { // Q: E = R[ra, rb, n], out[la, lb, s, t, n]
            d.La = (int)ra, d.Lb = (int)rb, d.C = (int)la, d.D = (int)lb;
            d.ea = 1, d.eb = (long long)ra, d.en = (long long)(ra * rb);
            d.aa = a_r, d.ac = a_l, d.bb = b_r, d.bd = b_l;
            d.oc = 1, d.od = (long long)la, d.os = (long long)(la * lb), d.ot = (long long)(la * lb * s), d.on = (long long)(la * lb * s * t);
        }
        return d;
    }

    // the half product of a gap site with pass-through bond m of the operator: P[n, x, a, d] from E = L[n, a, b], or Q[a, b, x, n] from
    // E = R[a, d, n], in the layouts partial_half_desc gives the same outputs (t = 1, the operator's bonds la = ra = m)
    static ApplyGapHalfDesc gap_half_desc(bool right, const double* env, size_t n_env, size_t m, const DevCore& X, double* out)
    {
        ApplyGapHalfDesc d{};
        const size_t lb = X.l, s = X.s, rb = X.r;
        d.E = env;
        d.X = X.buf.get();
        d.out = out;
        d.N = (int)n_env, d.M = (int)m, d.S = (int)s;
        if (!right) {
            d.K = (int)lb, d.C = (int)rb;
            d.en = 1, d.ea = (long long)n_env, d.ek = (long long)(n_env * m);
            d.xk = 1, d.xx = (long long)lb, d.xc = (long long)(lb * s);
            d.on = 1, d.ox = (long long)n_env, d.oa = (long long)(n_env * s), d.oc = (long long)(n_env * s * m);
        } else {
            d.K = (int)rb, d.C = (int)lb;
            d.ea = 1, d.ek = (long long)m, d.en = (long long)(m * rb);
            d.xk = (long long)(lb * s), d.xx = (long long)lb, d.xc = 1;
            d.oa = 1, d.oc = (long long)m, d.ox = (long long)(m * lb), d.on = (long long)(m * lb * s);
        }
        return d;
    }

    // the half product of site i of a plan into device memory that holds it
    void half_into(const Mpo& a, const Mpo& b, size_t i, bool right, const double* env, size_t n_env, double* out, const char* what)
    {
        const DevCore& A = a.tt.cores[i];
        const DevCore& B = b.tt.cores[i];
        const PartialSitePlan& p = (*plan)[i];
        const std::string where = what + std::to_string(i);
        check_count(n_env * p.S, p.T, right ? A.l : A.r, right ? B.l : B.r, where);
        check_count(n_env, A.l, B.l, 1, where);
        check_count(n_env, A.r, B.r, 1, where);
        if (gaps && (*gaps)[i].kind != ApplySiteKind::Op) {
            if (!apply_gap_half_launch(gap_half_desc(right, env, n_env, A.l, B, out), st))
                throw Error(T4A_GPU_INVALID_ARGUMENT, where + " needs more than INT_MAX workgroups");
            return;
        }
        if (!mpo_partial_half_launch(partial_half_desc(right, env, n_env, A, B, p, out), st))
            throw Error(T4A_GPU_INVALID_ARGUMENT, where + " needs more than INT_MAX workgroups");
    }

    // one half product of site i into `out`: P_i from L_i (n_env = c_i) or Q_i from R_{i+1} (n_env = c_{i+1})
    void half(const Mpo& a, const Mpo& b, size_t i, bool right, const double* env, size_t n_env, DevBuf<double>& out,
              const char* what = "contract_fit: site ")
    {
        const DevCore& A = a.tt.cores[i];
        const DevCore& B = b.tt.cores[i];
        if (plan) {
            check_count(n_env * (*plan)[i].S, (*plan)[i].T, right ? A.l : A.r, right ? B.l : B.r, what + std::to_string(i));
            out.reserve(n_env * st_dim(a, b, i) * (right ? A.l * B.l : A.r * B.r));
            half_into(a, b, i, right, env, n_env, out.get(), what);
            return;
        }
        const size_t S1 = a.sd[i][0], K = a.sd[i][1], T = b.sd[i][1];
        const std::string where = what + std::to_string(i);
        check_count(n_env * S1, T, right ? A.l : A.r, right ? B.l : B.r, where);
        check_count(n_env, A.l, B.l, 1, where);
        check_count(n_env, A.r, B.r, 1, where);
        out.reserve(n_env * S1 * T * (right ? A.l * B.l : A.r * B.r));
        if (!mpo_fit_half_launch(half_desc(right, env, n_env, A.buf.get(), A.l, S1, K, A.r, B.buf.get(), B.l, T, B.r, out.get()), st))
            throw Error(T4A_GPU_INVALID_ARGUMENT, where + " needs more than INT_MAX workgroups");
    }

    // R_i = Q_i C_i^T over (s, t, c_{i+1}), with C_i given as the c_i x (s t c_{i+1}) matrix `rows` of leading dimension ld
    void right_env(const Mpo& a, const Mpo& b, size_t i, size_t ci, size_t cnext, const double* rows, int ld)
    {
        const size_t ab = a.tt.cores[i].l * b.tt.cores[i].l, rest = st_dim(a, b, i) * cnext;
        envR[i].reserve(ab * ci);
        GemmDesc g = gemm_desc((int)ab, (int)ci, (int)rest, hq.get(), (int)ab, rows, ld, envR[i].get(), (int)ab);
        g.transB = 1;
        gemm_launch(g, st);
    }

    // The sweeps.  `c` is the start (any bonds); it leaves as the fitted MPO with its orthogonality centre on site 0.
    void fit(const Mpo& a, const Mpo& b, std::vector<DevCore>& c, size_t max_sweeps, double convergence_tol, MpoFitInfo& info)
    {
        const size_t n = c.size();
        sweeper.canonicalize(c, 0);
        envL.resize(n);
        envR.resize(n + 1);
        envL[0].reserve(1);
        envR[n].reserve(1);
        fill_launch(envL[0].get(), 1, 1.0, st);
        fill_launch(envR[n].get(), 1, 1.0, st);
        for (size_t i = n - 1; i >= 2; --i) {
            half(a, b, i, true, envR[i + 1].get(), c[i].r, hq);
            right_env(a, b, i, c[i].l, c[i].r, c[i].buf.get(), (int)c[i].l);
        }
        const std::vector<double> h0 = to_host(eng, c[0].buf.get(), c[0].size());
        double norm_prev = 0.0;
        for (double v : h0) norm_prev = std::hypot(norm_prev, v);
        info.norms.push_back(norm_prev);

        auto bond_step = [&](size_t i, bool move_right) {
            const size_t ci = c[i].l, cn = c[i + 1].r;
            const size_t sl = c[i].s, sr = c[i + 1].s; // s t of the two sites
            const size_t ab = a.tt.cores[i + 1].l * b.tt.cores[i + 1].l;
            half(a, b, i, false, envL[i].get(), ci, hp);
            half(a, b, i + 1, true, envR[i + 2].get(), cn, hq);
            const int M = (int)(ci * sl), N = (int)(sr * cn);
            check_count(ci * sl, sr * cn, 1, 1, "contract_fit: bond " + std::to_string(i));
            theta.reserve((size_t)M * N);
            gemm_launch(gemm_desc(M, N, (int)ab, hp.get(), M, hq.get(), (int)ab, theta.get(), M), st);
            const size_t rank = svd_rank(theta.get(), M, N);
            const int kmin = std::min(M, N);
            DevCore nl = DevCore::make(ci, sl, rank), nr = DevCore::make(rank, sr, cn);
            split_two_site(st, u.get(), M, s.get(), vt.get(), kmin, N, (int)rank, move_right, nl, nr);
            if (move_right) { // C_i = U, C_{i+1} = diag(S) Vt, L_{i+1} = U^T P_i
                envL[i + 1].reserve(rank * ab);
                GemmDesc g = gemm_desc((int)rank, (int)ab, M, u.get(), M, hp.get(), M, envL[i + 1].get(), (int)rank);
                g.transA = 1;
                gemm_launch(g, st);
            } else { // C_i = U diag(S), C_{i+1} = Vt, R_{i+1} = Q_{i+1} Vt^T
                right_env(a, b, i + 1, rank, cn, vt.get(), kmin);
            }
            T4A_HIP(hipGetLastError());
            eng.sync(); // the old sites are released below; u / s / vt are overwritten by the next step
            c[i] = std::move(nl);
            c[i + 1] = std::move(nr);
            double nrm = 0.0;
            for (size_t j = 0; j < rank; ++j) nrm = std::hypot(nrm, hs[j]);
            return nrm;
        };

        for (size_t sweep = 1; sweep <= max_sweeps; ++sweep) {
            double nrm = 0.0;
            for (size_t i = 0; i + 1 < n; ++i) nrm = bond_step(i, true);
            for (size_t i = n - 1; i-- > 0;) nrm = bond_step(i, false);
            info.norms.push_back(nrm);
            info.n_sweeps = sweep;
            const bool converged = std::fabs(nrm / norm_prev - 1.0) < convergence_tol; // a zero product: 0 / 0 is NaN, never converged
            norm_prev = nrm;
            if (converged) break;
        }
    }
};

} // namespace

void mpo_validate_dims(const std::vector<std::array<size_t, 4>>& d)
{
    const size_t n = d.size();
    for (size_t i = 0; i + 1 < n; ++i)
        if (d[i][3] != d[i + 1][0])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Bond shape mismatch at site " + std::to_string(i) + ": left tensor has right_dim=" +
                                                      std::to_string(d[i][3]) + ", right tensor has left_dim=" + std::to_string(d[i + 1][0]));
    if (n && (d[0][0] != 1 || d[n - 1][3] != 1))
        throw Error(T4A_GPU_INVALID_ARGUMENT,
                    "Invalid boundary conditions: first tensor must have left_dim=1, last tensor must have right_dim=1");
    for (size_t i = 0; i < n; ++i) {
        const std::string site = "MPO site " + std::to_string(i);
        for (size_t x : d[i])
            if (x == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, site + " has a zero dimension");
        check_count(d[i][0], d[i][1], d[i][2], d[i][3], site);
        if (d[i][0] > MPO_DIM_MAX || d[i][3] > MPO_DIM_MAX || d[i][1] * d[i][2] > MPO_DIM_MAX)
            throw Error(T4A_GPU_INVALID_ARGUMENT, site + ": dimensions above 65535 are not supported");
    }
}

namespace {
std::vector<std::array<size_t, 3>> fused(const std::vector<std::array<size_t, 4>>& d)
{
    mpo_validate_dims(d);
    std::vector<std::array<size_t, 3>> f(d.size());
    for (size_t i = 0; i < d.size(); ++i) f[i] = {d[i][0], d[i][1] * d[i][2], d[i][3]};
    return f;
}
std::vector<std::array<size_t, 2>> pairs(const std::vector<std::array<size_t, 4>>& d)
{
    std::vector<std::array<size_t, 2>> p(d.size());
    for (size_t i = 0; i < d.size(); ++i) p[i] = {d[i][1], d[i][2]};
    return p;
}
} // namespace

Mpo::Mpo(const std::vector<std::array<size_t, 4>>& dims4, const double* host_data) : tt(fused(dims4), host_data), sd(pairs(dims4)) {}

Mpo::Mpo(const std::vector<DevCore>& cores, hipStream_t src_stream, const std::vector<std::array<size_t, 2>>& site_dims)
    : tt(cores, src_stream), sd(site_dims)
{
}

Mpo::Mpo(std::vector<DevCore>&& cores, const std::vector<std::array<size_t, 2>>& site_dims) : tt(std::vector<DevCore>{}, nullptr), sd(site_dims)
{
    tt.cores = std::move(cores);
}

std::vector<std::array<size_t, 4>> Mpo::dims4() const
{
    std::vector<std::array<size_t, 4>> d(len());
    for (size_t i = 0; i < len(); ++i) d[i] = {tt.cores[i].l, sd[i][0], sd[i][1], tt.cores[i].r};
    return d;
}

std::vector<double> Mpo::evaluate(const uint32_t* idx, size_t n_pts)
{
    const size_t n = len();
    if (n == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "MPO is empty");
    std::vector<uint32_t> f(n * n_pts);
    for (size_t p = 0; p < n_pts; ++p)
        for (size_t s = 0; s < n; ++s) {
            const uint32_t i = idx[2 * n * p + 2 * s], j = idx[2 * n * p + 2 * s + 1];
            if (i >= sd[s][0] || j >= sd[s][1])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "Index out of bounds: index " + std::to_string(std::max(i, j)) + " at site " +
                                                          std::to_string(s) + " (max: " + std::to_string(std::max(sd[s][0], sd[s][1])) + ")");
            f[n * p + s] = i + (uint32_t)sd[s][0] * j; // the fused index of the train
        }
    return tt.evaluate(f.data(), n_pts);
}

std::unique_ptr<Mpo> Mpo::transpose()
{
    const size_t n = len();
    std::vector<DevCore> out(n);
    std::vector<std::array<size_t, 2>> tsd(n);
    const hipStream_t st = tt.eng.stream();
    for (size_t i = 0; i < n; ++i) {
        const DevCore& c = tt.cores[i];
        out[i] = DevCore::make(c.l, c.s, c.r);
        tsd[i] = {sd[i][1], sd[i][0]};
        const size_t d[4] = {c.l, sd[i][0], sd[i][1], c.r}, p[4] = {0, 2, 1, 3};
        permute_launch(c.buf.get(), d, p, 4, out[i].buf.get(), st);
    }
    T4A_HIP(hipGetLastError());
    tt.eng.sync();
    return std::make_unique<Mpo>(std::move(out), tsd);
}

void Mpo::relabel_site_dims(const std::vector<std::array<size_t, 2>>& site_dims)
{
    if (site_dims.size() != len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "relabel_site_dims: one (s1, s2) pair per site is needed");
    for (size_t i = 0; i < len(); ++i)
        if (site_dims[i][0] * site_dims[i][1] != tt.cores[i].s)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "relabel_site_dims: site " + std::to_string(i) + " has " + std::to_string(tt.cores[i].s) +
                                                      " fused indices, not " + std::to_string(site_dims[i][0]) + " * " +
                                                      std::to_string(site_dims[i][1]));
    sd = site_dims;
}

namespace {
// the shape checks of contract_naive / contract_zipup / contract_fit (contract_fit.rs:74-92)
void check_operands(const Mpo& a, const Mpo& b)
{
    if (a.len() != b.len())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "MPO length mismatch: expected " + std::to_string(a.len()) + ", got " + std::to_string(b.len()));
    for (size_t i = 0; i < a.len(); ++i)
        if (a.sd[i][1] != b.sd[i][0])
            throw Error(T4A_GPU_INVALID_ARGUMENT, "Shared shape mismatch at site " + std::to_string(i) + ": MPO A has site_dim_2=" +
                                                      std::to_string(a.sd[i][1]) + ", MPO B has site_dim_1=" + std::to_string(b.sd[i][0]));
}
} // namespace

std::unique_ptr<Mpo> mpo_contract(Mpo& a, Mpo& b, MpoAlgorithm alg, bool compress, const MpoContractionOptions& opt)
{
    check_operands(a, b);
    const size_t n = a.len();
    if (alg == MpoAlgorithm::Fit) // contract_fit.rs:65-96
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "Unsupported operation: simplett variational MPO fitting is not implemented; use contract_naive or "
                                             "contract_zipup instead");
    std::vector<std::array<size_t, 2>> sd(n);
    for (size_t i = 0; i < n; ++i) sd[i] = {a.sd[i][0], b.sd[i][1]};
    if (n == 0) return std::make_unique<Mpo>(std::vector<DevCore>{}, sd);
    b.tt.eng.sync(); // b's cores are read on a's stream (TensorTrain::add)
    Contractor c(a.tt.eng, opt);
    std::vector<DevCore> cores;
    if (alg == MpoAlgorithm::ZipUp) {
        cores = c.zipup(a, b);
    } else {
        cores = c.naive(a, b);
        if (compress) c.compress(cores);
    }
    a.tt.eng.sync();
    return std::make_unique<Mpo>(std::move(cores), sd);
}

void mpo_compress_cores(Engine& eng, std::vector<DevCore>& cores, const MpoContractionOptions& opt)
{
    Contractor c(eng, opt);
    c.compress(cores);
    eng.sync();
}

void mpo_fit_validate_options(const MpoFitOptions& opt)
{
    if (!(opt.tolerance >= 0.0) || !std::isfinite(opt.tolerance))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "contract_fit: tolerance must be finite and not negative");
    if (!(opt.convergence_tol >= 0.0) || !std::isfinite(opt.convergence_tol))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "contract_fit: convergence_tol must be finite and not negative");
}

namespace {
// what mpo_contract_fit and mpo_partial_contract_fit share behind their shape checks: `sd` are the site dims of the product, `plan` the
// site plans of a partial contraction or null for the matrix product
std::unique_ptr<Mpo> fit_driver(Mpo& a, Mpo& b, const std::vector<PartialSitePlan>* plan, const std::vector<std::array<size_t, 2>>& sd,
                                const MpoFitOptions& opt, Mpo* initial, MpoFitInfo& info)
{
    const size_t n = a.len();
    if (initial) {
        if (initial->len() != n)
            throw Error(T4A_GPU_INVALID_ARGUMENT,
                        "contract_fit: initial has " + std::to_string(initial->len()) + " sites, the product has " + std::to_string(n));
        for (size_t i = 0; i < n; ++i)
            if (initial->sd[i] != sd[i])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "contract_fit: initial has site dims (" + std::to_string(initial->sd[i][0]) + ", " +
                                                          std::to_string(initial->sd[i][1]) + ") at site " + std::to_string(i) +
                                                          ", the product has (" + std::to_string(sd[i][0]) + ", " + std::to_string(sd[i][1]) + ")");
    }
    mpo_fit_validate_options(opt);
    if (n == 0) return std::make_unique<Mpo>(std::vector<DevCore>{}, sd);
    b.tt.eng.sync(); // b's and initial's cores are read on a's stream
    if (initial) initial->tt.eng.sync();
    MpoContractionOptions co;
    co.tolerance = opt.tolerance;
    co.max_bond_dim = opt.max_bond_dim;
    co.method = opt.method;
    Contractor c(a.tt.eng, co);
    c.plan = plan;
    std::vector<DevCore> cores;
    if (n == 1) { // the exact one-site product, nothing to sweep
        cores = plan ? c.naive_partial(a, b) : c.naive(a, b);
    } else {
        if (initial) {
            cores = clone_cores(initial->tt.cores, c.st);
        } else {
            cores = plan ? c.zipup_partial(a, b) : c.zipup(a, b); // the initialiser of treetn::contract_fit, same tolerance, cap and method
        }
        if (opt.max_sweeps > 0) c.fit(a, b, cores, opt.max_sweeps, opt.convergence_tol, info);
    }
    a.tt.eng.sync();
    return std::make_unique<Mpo>(std::move(cores), sd);
}
} // namespace

std::unique_ptr<Mpo> mpo_contract_fit(Mpo& a, Mpo& b, const MpoFitOptions& opt, Mpo* initial, MpoFitInfo& info)
{
    info = MpoFitInfo{};
    check_operands(a, b);
    std::vector<std::array<size_t, 2>> sd(a.len());
    for (size_t i = 0; i < a.len(); ++i) sd[i] = {a.sd[i][0], b.sd[i][1]};
    return fit_driver(a, b, nullptr, sd, opt, initial, info);
}

std::vector<double> mpo_fit_half(const double* env, size_t n_env, bool right, Mpo& a, Mpo& b, size_t site)
{
    check_operands(a, b);
    if (site >= a.len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "fit_half: site " + std::to_string(site) + " is out of range");
    if (n_env == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "fit_half: the environment has a zero dimension");
    const DevCore& A = a.tt.cores[site];
    const DevCore& B = b.tt.cores[site];
    const size_t ea = right ? A.r : A.l, eb = right ? B.r : B.l, oa = right ? A.l : A.r, ob = right ? B.l : B.r;
    check_count(n_env, ea, eb, 1, "fit_half: the environment");
    check_count(n_env * a.sd[site][0], b.sd[site][1], oa, ob, "fit_half: the half product");
    b.tt.eng.sync();
    MpoContractionOptions co;
    Contractor c(a.tt.eng, co);
    DevBuf<double> d_env, d_out;
    const size_t ne = n_env * ea * eb, no = n_env * a.sd[site][0] * b.sd[site][1] * oa * ob;
    d_env.reserve(ne);
    T4A_HIP(hipMemcpyAsync(d_env.get(), env, sizeof(double) * ne, hipMemcpyHostToDevice, c.st));
    c.half(a, b, site, right, d_env.get(), n_env, d_out);
    T4A_HIP(hipGetLastError());
    return to_host(a.tt.eng, d_out.get(), no);
}

// ---- partial contraction (mpo.hpp) ----
std::vector<PartialSitePlan> mpo_partial_plan(const std::vector<std::array<size_t, 2>>& a_sd, const std::vector<std::array<size_t, 2>>& b_sd,
                                              const PartialSpec& spec)
{
    if (a_sd.size() != b_sd.size())
        throw Error(T4A_GPU_INVALID_ARGUMENT, "MPO length mismatch: expected " + std::to_string(a_sd.size()) + ", got " + std::to_string(b_sd.size()));
    const size_t n = a_sd.size();
    enum Role : int { Free = 0, Contract = 1, Diagonal = 2 };
    struct Leg {
        Role role = Free;
        size_t partner = 0; // the leg of the other operand at the same site
    };
    std::vector<std::array<Leg, 2>> ra(n), rb(n);
    std::vector<std::array<bool, 2>> seen_a(n, {false, false}), seen_b(n, {false, false});
    auto name = [](size_t site, size_t leg) { return "(site " + std::to_string(site) + ", leg " + std::to_string(leg) + ")"; };
    const PartialPair* cross = nullptr;
    for (int kind = 0; kind < 2; ++kind) {
        const std::string kname = kind == 0 ? "contract_pairs" : "diagonal_pairs";
        for (const PartialPair& p : kind == 0 ? spec.contract_pairs : spec.diagonal_pairs) {
            if (p.site_a >= n || p.leg_a > 1)
                throw Error(T4A_GPU_INVALID_ARGUMENT,
                            "partial_contract: " + name(p.site_a, p.leg_a) + " from " + kname + " not found in first MPO external indices");
            if (p.site_b >= n || p.leg_b > 1)
                throw Error(T4A_GPU_INVALID_ARGUMENT,
                            "partial_contract: " + name(p.site_b, p.leg_b) + " from " + kname + " not found in second MPO external indices");
            const size_t da = a_sd[p.site_a][p.leg_a], db = b_sd[p.site_b][p.leg_b];
            if (da != db)
                throw Error(T4A_GPU_INVALID_ARGUMENT,
                            "partial_contract: " + kname + " index shape mismatch: " + std::to_string(da) + " != " + std::to_string(db));
            if (seen_a[p.site_a][p.leg_a])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "partial_contract: first MPO index " + name(p.site_a, p.leg_a) + " appears in multiple pairs");
            if (seen_b[p.site_b][p.leg_b])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "partial_contract: second MPO index " + name(p.site_b, p.leg_b) + " appears in multiple pairs");
            seen_a[p.site_a][p.leg_a] = seen_b[p.site_b][p.leg_b] = true;
            if (p.site_a != p.site_b) {
                if (!cross) cross = &p;
                continue;
            }
            ra[p.site_a][p.leg_a] = Leg{kind == 0 ? Contract : Diagonal, p.leg_b};
            rb[p.site_b][p.leg_b] = Leg{kind == 0 ? Contract : Diagonal, p.leg_a};
        }
    }
    if (cross)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "partial_contract: the pair " + name(cross->site_a, cross->leg_a) + " - " +
                                                 name(cross->site_b, cross->leg_b) +
                                                 " joins two sites; moving a site index (swap_site_indices) is not implemented");
    if (spec.has_output_order)
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "partial_contract: output_order is not implemented (it needs swap_site_indices)");
    std::vector<PartialSitePlan> plan(n);
    for (size_t i = 0; i < n; ++i) {
        PartialSitePlan& p = plan[i];
        const size_t stride_a[2] = {1, a_sd[i][0]}, stride_b[2] = {1, b_sd[i][0]};
        size_t ns = 0, nk = 0, nt = 0;
        for (size_t leg = 0; leg < 2; ++leg) {
            const Leg& l = ra[i][leg];
            const size_t dim = a_sd[i][leg];
            if (l.role == Contract) {
                p.ak[nk] = stride_a[leg];
                p.bk[nk] = stride_b[l.partner];
                if (nk == 0) p.k0 = dim;
                p.K *= dim;
                ++nk;
            } else {
                p.as[ns] = stride_a[leg];
                p.bs[ns] = l.role == Diagonal ? stride_b[l.partner] : 0;
                if (ns == 0) p.s0 = dim;
                p.S *= dim;
                p.leg_dims[ns] = dim;
                ++ns;
            }
        }
        for (size_t leg = 0; leg < 2; ++leg) {
            if (rb[i][leg].role != Free) continue;
            const size_t dim = b_sd[i][leg];
            p.bt[nt] = stride_b[leg];
            if (nt == 0) p.t0 = dim;
            p.T *= dim;
            p.leg_dims[2 + nt] = dim;
            ++nt;
        }
        if (p.S == 0 || p.T == 0 || p.K == 0)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "partial_contract: site " + std::to_string(i) + " has a zero dimension");
        check_count(p.S, p.T, 1, 1, "partial_contract: site " + std::to_string(i));
        if (p.S * p.T > MPO_DIM_MAX)
            throw Error(T4A_GPU_INVALID_ARGUMENT, "partial_contract: site " + std::to_string(i) + ": dimensions above 65535 are not supported");
    }
    return plan;
}

namespace {
std::vector<PartialSitePlan> plan_of(const Mpo& a, const Mpo& b, const PartialSpec& spec) { return mpo_partial_plan(a.sd, b.sd, spec); }
std::vector<std::array<size_t, 2>> plan_site_dims(const std::vector<PartialSitePlan>& plan)
{
    std::vector<std::array<size_t, 2>> sd(plan.size());
    for (size_t i = 0; i < plan.size(); ++i) sd[i] = {plan[i].S, plan[i].T};
    return sd;
}
} // namespace

std::unique_ptr<Mpo> mpo_partial_contract(Mpo& a, Mpo& b, const PartialSpec& spec, MpoAlgorithm alg, bool compress,
                                          const MpoContractionOptions& opt)
{
    const std::vector<PartialSitePlan> plan = plan_of(a, b, spec);
    const size_t n = a.len();
    if (alg == MpoAlgorithm::Fit) // as mpo_contract
        throw Error(T4A_GPU_NOT_IMPLEMENTED, "Unsupported operation: simplett variational MPO fitting is not implemented; use contract_naive or "
                                             "contract_zipup instead");
    const std::vector<std::array<size_t, 2>> sd = plan_site_dims(plan);
    if (n == 0) return std::make_unique<Mpo>(std::vector<DevCore>{}, sd);
    b.tt.eng.sync(); // b's cores are read on a's stream
    Contractor c(a.tt.eng, opt);
    c.plan = &plan;
    std::vector<DevCore> cores;
    if (alg == MpoAlgorithm::ZipUp) {
        cores = c.zipup_partial(a, b);
    } else {
        cores = c.naive_partial(a, b);
        if (compress) c.compress(cores);
    }
    a.tt.eng.sync();
    return std::make_unique<Mpo>(std::move(cores), sd);
}

std::unique_ptr<Mpo> mpo_partial_contract_fit(Mpo& a, Mpo& b, const PartialSpec& spec, const MpoFitOptions& opt, Mpo* initial, MpoFitInfo& info)
{
    info = MpoFitInfo{};
    const std::vector<PartialSitePlan> plan = plan_of(a, b, spec);
    return fit_driver(a, b, &plan, plan_site_dims(plan), opt, initial, info);
}

std::vector<double> mpo_partial_half(const double* env, size_t n_env, bool right, Mpo& a, Mpo& b, const PartialSpec& spec, size_t site)
{
    const std::vector<PartialSitePlan> plan = plan_of(a, b, spec);
    if (site >= a.len()) throw Error(T4A_GPU_INVALID_ARGUMENT, "partial_half: site " + std::to_string(site) + " is out of range");
    if (n_env == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "partial_half: the environment has a zero dimension");
    const DevCore& A = a.tt.cores[site];
    const DevCore& B = b.tt.cores[site];
    const size_t ea = right ? A.r : A.l, eb = right ? B.r : B.l, oa = right ? A.l : A.r, ob = right ? B.l : B.r;
    check_count(n_env, ea, eb, 1, "partial_half: the environment");
    check_count(n_env * plan[site].S, plan[site].T, oa, ob, "partial_half: the half product");
    b.tt.eng.sync();
    MpoContractionOptions co;
    Contractor c(a.tt.eng, co);
    c.plan = &plan;
    DevBuf<double> d_env, d_out;
    const size_t ne = n_env * ea * eb, no = n_env * plan[site].S * plan[site].T * oa * ob;
    d_env.reserve(ne);
    T4A_HIP(hipMemcpyAsync(d_env.get(), env, sizeof(double) * ne, hipMemcpyHostToDevice, c.st));
    c.half(a, b, site, right, d_env.get(), n_env, d_out, "partial_half: site ");
    T4A_HIP(hipGetLastError());
    return to_host(a.tt.eng, d_out.get(), no);
}

// ---- an operator on a subset of the state's sites, fused route (linop.hpp) ----
namespace {
// A chain of cores that belong to somebody else, read as an MPO for the length of one contraction: nothing is copied and nothing is
// released.  A core without a buffer is a shape only (the operator at a gap site).  A borrowed pointer never sits in a DevCore outside
// this object, whose destructor forgets it before the DevBuf could hand it to the pool.
struct BorrowedMpo {
    Mpo m;
    BorrowedMpo(size_t n, const std::vector<std::array<size_t, 2>>& sd) : m(std::vector<DevCore>(n), sd) {}
    BorrowedMpo(const BorrowedMpo&) = delete;
    BorrowedMpo& operator=(const BorrowedMpo&) = delete;
    ~BorrowedMpo()
    {
        for (DevCore& c : m.tt.cores) c.buf.p = nullptr, c.buf.cap = 0, c.buf.bytes_ = 0;
    }
    void view(size_t i, double* p, size_t l, size_t s, size_t r)
    {
        DevCore& c = m.tt.cores[i];
        c.buf.p = p;
        c.buf.cap = p ? l * s * r : 0;
        c.l = l, c.s = s, c.r = r;
    }
};
} // namespace

std::unique_ptr<Mpo> linop_fused_contract(Mpo& op, TensorTrain& state, const std::vector<ApplySitePlan>& ap, bool fit, const MpoFitOptions& opt,
                                          Mpo* initial, MpoFitInfo& info)
{
    info = MpoFitInfo{};
    const size_t n = state.len();
    std::vector<std::array<size_t, 2>> sd(n), a_sd(n), b_sd(n);
    PartialSpec spec;
    for (size_t i = 0; i < n; ++i) {
        sd[i] = {ap[i].d_out, 1};
        a_sd[i] = {ap[i].d_out, ap[i].d_in};
        b_sd[i] = {ap[i].d_in, 1};
        spec.contract_pairs.push_back(PartialPair{i, 1, i, 0});
    }
    BorrowedMpo a(n, a_sd), b(n, b_sd);
    for (size_t i = 0; i < n; ++i) {
        const ApplySitePlan& p = ap[i];
        const DevCore& X = state.cores[i];
        a.view(i, p.kind == ApplySiteKind::Op ? op.tt.cores[p.op_site].buf.get() : nullptr, p.m_left, p.d_out * p.d_in, p.m_right);
        b.view(i, X.buf.get(), X.l, X.s, X.r);
    }
    const std::vector<PartialSitePlan> plan = mpo_partial_plan(a_sd, b_sd, spec); // the matrix-product plan: S = d_out, K = d_in, T = 1
    if (initial) {
        if (initial->len() != n)
            throw Error(T4A_GPU_INVALID_ARGUMENT,
                        "apply_linear_operator: initial has " + std::to_string(initial->len()) + " sites, the result has " + std::to_string(n));
        for (size_t i = 0; i < n; ++i)
            if (initial->sd[i] != sd[i])
                throw Error(T4A_GPU_INVALID_ARGUMENT, "apply_linear_operator: initial has site dim " + std::to_string(initial->sd[i][0]) + " at site " +
                                                          std::to_string(i) + ", the result has " + std::to_string(sd[i][0]));
    }
    mpo_fit_validate_options(opt);
    if (n == 0) return std::make_unique<Mpo>(std::vector<DevCore>{}, sd);
    op.tt.eng.sync(); // the operands' cores are read on the stream of the view
    state.eng.sync();
    if (initial) initial->tt.eng.sync();
    MpoContractionOptions co;
    co.tolerance = opt.tolerance;
    co.max_bond_dim = opt.max_bond_dim;
    co.method = opt.method;
    Contractor c(a.m.tt.eng, co);
    c.plan = &plan;
    c.gaps = &ap;
    std::vector<DevCore> cores;
    if (fit && initial) cores = clone_cores(initial->tt.cores, c.st);
    else cores = c.zipup_partial(a.m, b.m);
    if (fit && n > 1 && opt.max_sweeps > 0) c.fit(a.m, b.m, cores, opt.max_sweeps, opt.convergence_tol, info);
    a.m.tt.eng.sync();
    return std::make_unique<Mpo>(std::move(cores), sd);
}

std::vector<double> apply_gap_half(bool right, const double* env, size_t n_env, size_t m, const double* x, size_t lb, size_t d, size_t rb,
                                   const double* fill, size_t guard)
{
    if (n_env == 0 || m == 0 || lb == 0 || d == 0 || rb == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "linop_gap_half: a dimension is zero");
    const size_t k = right ? rb : lb, c = right ? lb : rb;
    check_count(n_env, m, k, 1, "linop_gap_half: the environment");
    check_count(lb, d, rb, 1, "linop_gap_half: the site");
    check_count(n_env * d, m, c, 1, "linop_gap_half: the half product");
    Engine eng;
    const hipStream_t st = eng.stream();
    DevBuf<double> d_env, d_out;
    DevCore X = DevCore::make(lb, d, rb);
    const size_t ne = n_env * m * k, no = n_env * d * m * c;
    d_env.reserve(ne);
    d_out.reserve(no + guard);
    T4A_HIP(hipMemcpyAsync(d_env.get(), env, sizeof(double) * ne, hipMemcpyHostToDevice, st));
    T4A_HIP(hipMemcpyAsync(X.buf.get(), x, sizeof(double) * X.size(), hipMemcpyHostToDevice, st));
    if (fill) fill_launch(d_out.get(), no + guard, *fill, st);
    if (!apply_gap_half_launch(Contractor::gap_half_desc(right, d_env.get(), n_env, m, X, d_out.get()), st))
        throw Error(T4A_GPU_INVALID_ARGUMENT, "linop_gap_half needs more than INT_MAX workgroups");
    T4A_HIP(hipGetLastError());
    return to_host(eng, d_out.get(), fill ? no + guard : no);
}

void linop_time_half(size_t n_env, size_t m, size_t lb, size_t d, size_t rb, size_t reps, double ms[2])
{
    if (reps == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "linop_time_half: reps must be positive");
    if (n_env == 0 || m == 0 || lb == 0 || d == 0 || rb == 0) throw Error(T4A_GPU_INVALID_ARGUMENT, "linop_time_half: a dimension is zero");
    check_count(n_env, m, lb, 1, "linop_time_half: the environment");
    check_count(lb, d, rb, 1, "linop_time_half: the site");
    check_count(m, d, d, m, "linop_time_half: the bridge site");
    check_count(n_env * d, m, rb, 1, "linop_time_half: the half product");
    Engine eng;
    const hipStream_t st = eng.stream();
    DevBuf<double> d_env, d_out;
    DevCore X = DevCore::make(lb, d, rb), O = DevCore::make(m, d * d, m);
    d_env.reserve(n_env * m * lb);
    d_out.reserve(n_env * d * m * rb);
    fill_launch(d_env.get(), n_env * m * lb, 0.5, st); // constant operands: the time does not depend on the values
    fill_launch(X.buf.get(), X.size(), 0.25, st);
    fill_launch(O.buf.get(), O.size(), 1.0, st);
    PartialSitePlan p; // the matrix-product plan of O[m, d, d, m] on X[lb, d, 1, rb]
    p.S = p.s0 = d, p.K = p.k0 = d, p.T = p.t0 = 1;
    p.as[0] = 1, p.ak[0] = d, p.bk[0] = 1;
    const std::function<void()> pieces[2] = {
        [&] { apply_gap_half_launch(Contractor::gap_half_desc(false, d_env.get(), n_env, m, X, d_out.get()), st); },
        [&] { mpo_partial_half_launch(Contractor::partial_half_desc(false, d_env.get(), n_env, O, X, p, d_out.get()), st); },
    };
    time_pieces(st, pieces, 2, reps, ms);
    T4A_HIP(hipGetLastError());
    eng.sync();
}

} // namespace t4a
