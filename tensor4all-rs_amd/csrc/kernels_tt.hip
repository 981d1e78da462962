// kernels_tt.hip — tensor-train kernels next to the TCI2 sweep (SURVEY.md §8 rows a15–a18):
//   core <-> left/right matrix reshapes   <- tensor3_to_left_matrix / tensor3_to_right_matrix / split_indices
//                                            (simplett/src/compression.rs:127-161, tensorci/src/conversion.rs:273-351)
//   sum, norm2                             <- AbstractTensorTrain::sum / norm2 (simplett/src/traits.rs:231-354)
//   left / right environments + dots       <- TTCache::evaluate_left / evaluate_right / evaluate_many
//                                            (simplett/src/cache.rs:430-688, einsum_helper.rs:192-268)
//   generic axis permutation               <- the dense tensor layer (tensorops.hip) and the zip-up MPO contraction (mpo.hip)
//   bond scaling, column scaling           <- the Vidal / inverse forms (simplett/src/vidal.rs:106-111, :364-388, :456-492, :551-663, :730-766)
// The chain contractions keep the reference's summation order (index ascending, separately rounded multiply and
// add; built with -ffp-contract=off), so their results are bit-identical to the CPU oracle's.
#include "kernels.hpp"

#include <algorithm>

namespace t4a {

namespace {

// mode 0: core -> left matrix  (row l*S+s, col r)      1: left matrix -> core
// mode 2: core -> right matrix (row l, col s*R+r)      3: right matrix -> core
__global__ void __launch_bounds__(256) core_reshape_kernel(const double* __restrict__ in, int L, int S, int R, int mode,
                                                           double* __restrict__ out)
{
    const size_t total = (size_t)L * S * R;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        // e enumerates the OUTPUT linearly
        size_t src;
        if (mode == 0) { // out = left matrix: e = (l*S+s) + L*S*r
            const size_t r = e / ((size_t)L * S), row = e % ((size_t)L * S);
            const size_t l = row / S, s = row % S;
            src = l + (size_t)L * (s + (size_t)S * r);
        } else if (mode == 1) { // out = core: e = l + L*(s + S*r)
            const size_t l = e % L, sr = e / L;
            const size_t s = sr % S, r = sr / S;
            src = (l * S + s) + (size_t)L * S * r;
        } else if (mode == 2) { // out = right matrix: e = l + L*(s*R + r)
            const size_t l = e % L, c = e / L;
            const size_t s = c / R, r = c % R;
            src = l + (size_t)L * (s + (size_t)S * r);
        } else { // out = core from right matrix
            const size_t l = e % L, sr = e / L;
            const size_t s = sr % S, r = sr / S;
            src = l + (size_t)L * (s * (size_t)R + r);
        }
        out[e] = in[src];
    }
}

// sum over all indices (traits.rs:231-275): cur[r] = sum_l cur[l] * (sum_s T[l,s,r]), single workgroup.
__global__ void __launch_bounds__(256) tt_sum_kernel(const TtCoreDesc* cores, int n_sites, int max_bond, double* out)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* cur = (double*)smem_raw;
    double* nxt = cur + max_bond;
    const int tid = threadIdx.x, T = blockDim.x;
    {
        const TtCoreDesc c0 = cores[0];
        for (int r = tid; r < c0.r; r += T) {
            double acc = 0.0;
            for (int s = 0; s < c0.d; ++s) acc = acc + c0.data[(size_t)c0.l * ((size_t)s + (size_t)c0.d * r)];
            cur[r] = acc;
        }
    }
    __syncthreads();
    for (int site = 1; site < n_sites; ++site) {
        const TtCoreDesc c = cores[site];
        for (int r = tid; r < c.r; r += T) {
            double sum = 0.0;
            for (int l = 0; l < c.l; ++l) {
                double ss = 0.0;
                for (int s = 0; s < c.d; ++s) ss = ss + c.data[(size_t)l + (size_t)c.l * ((size_t)s + (size_t)c.d * r)];
                const double prod = cur[l] * ss;
                sum = sum + prod;
            }
            nxt[r] = sum;
        }
        __syncthreads();
        double* t = cur;
        cur = nxt;
        nxt = t;
    }
    if (tid == 0) out[0] = cur[0];
}

// norm2 transfer step (traits.rs:314-347): nxt[ra*R+rc] = sum_{la,lc,s} (cur[la*L+lc] * T[la,s,ra]) * T[lc,s,rc]
// in the reference's loop order.  first != 0: cur is implicitly the 1x1 identity... the first site has its own
// form nxt[ra*R+rc] = sum_s T[0,s,ra]*T[0,s,rc] (traits.rs:298-309).
__global__ void __launch_bounds__(256) tt_norm2_step_kernel(TtCoreDesc c, const double* __restrict__ cur, int first,
                                                            double* __restrict__ nxt)
{
    const int R = c.r, L = c.l, S = c.d;
    const size_t total = (size_t)R * R;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int ra = (int)(e / R), rc = (int)(e % R);
        const double* ta = c.data + (size_t)L * S * ra;
        const double* tc = c.data + (size_t)L * S * rc;
        double acc = 0.0;
        if (first) {
            for (int s = 0; s < S; ++s) {
                const double prod = ta[(size_t)L * s] * tc[(size_t)L * s];
                acc = acc + prod;
            }
        } else {
            for (int la = 0; la < L; ++la)
                for (int lc = 0; lc < L; ++lc) {
                    const double cv = cur[(size_t)la * L + lc];
                    for (int s = 0; s < S; ++s) {
                        const double p1 = cv * ta[la + (size_t)L * s];
                        const double p2 = p1 * tc[lc + (size_t)L * s];
                        acc = acc + p2;
                    }
                }
        }
        nxt[e] = acc;
    }
}

// Left environments (cache.rs:430-467): one workgroup per prefix; env <- env * T_k[:, i_k, :] for k < split.
// idx: n_items x split (uint32, item-major); out: n_items x ld.
__global__ void __launch_bounds__(256) tt_env_left_kernel(const TtCoreDesc* cores, int split, int max_bond,
                                                          const uint32_t* __restrict__ idx, int n_items, double* out,
                                                          int ld)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* cur = (double*)smem_raw;
    double* nxt = cur + max_bond;
    const int tid = threadIdx.x, T = blockDim.x;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const uint32_t* my = idx + (size_t)it * split;
        {
            const TtCoreDesc c0 = cores[0];
            for (int r = tid; r < c0.r; r += T) cur[r] = c0.data[(size_t)c0.l * ((size_t)my[0] + (size_t)c0.d * r)];
        }
        __syncthreads();
        for (int s = 1; s < split; ++s) {
            const TtCoreDesc c = cores[s];
            for (int r = tid; r < c.r; r += T) {
                const double* col = c.data + (size_t)c.l * ((size_t)my[s] + (size_t)c.d * r);
                double sum = 0.0;
                for (int l = 0; l < c.l; ++l) {
                    const double prod = cur[l] * col[l];
                    sum = sum + prod;
                }
                nxt[r] = sum;
            }
            __syncthreads();
            double* t = cur;
            cur = nxt;
            nxt = t;
        }
        const int rl = cores[split - 1].r;
        for (int r = tid; r < rl; r += T) out[(size_t)it * ld + r] = cur[r];
        __syncthreads();
    }
}

// Right environments (cache.rs:469-518): env <- T_k[:, i_k, :] * env from the last site down to `split`.
// idx: n_items x (n_sites - split); out: n_items x ld.
__global__ void __launch_bounds__(256) tt_env_right_kernel(const TtCoreDesc* cores, int n_sites, int split, int max_bond,
                                                           const uint32_t* __restrict__ idx, int n_items, double* out,
                                                           int ld)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* cur = (double*)smem_raw;
    double* nxt = cur + max_bond;
    const int tid = threadIdx.x, T = blockDim.x;
    const int w = n_sites - split;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const uint32_t* my = idx + (size_t)it * w;
        {
            const TtCoreDesc cl = cores[n_sites - 1];
            // slice of the last site: (l, r = 0..cl.r), the chain requires cl.r == 1
            for (int l = tid; l < cl.l; l += T) cur[l] = cl.data[(size_t)l + (size_t)cl.l * (size_t)my[w - 1]];
        }
        __syncthreads();
        for (int s = n_sites - 2; s >= split; --s) {
            const TtCoreDesc c = cores[s];
            const uint32_t is = my[s - split];
            for (int l = tid; l < c.l; l += T) {
                double sum = 0.0;
                for (int r = 0; r < c.r; ++r) {
                    const double prod = c.data[(size_t)l + (size_t)c.l * ((size_t)is + (size_t)c.d * r)] * cur[r];
                    sum = sum + prod;
                }
                nxt[l] = sum;
            }
            __syncthreads();
            double* t = cur;
            cur = nxt;
            nxt = t;
        }
        const int ll = cores[split].l;
        for (int l = tid; l < ll; l += T) out[(size_t)it * ld + l] = cur[l];
        __syncthreads();
    }
}

// out[p] = sum_i left[il[p]][i] * right[ir[p]][i]  (cache.rs:668-685)
__global__ void __launch_bounds__(256) tt_env_dot_kernel(const double* __restrict__ left, const double* __restrict__ right,
                                                         int len, int ld, const uint32_t* __restrict__ il,
                                                         const uint32_t* __restrict__ ir, size_t n_pts, double* out)
{
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pts; p += (size_t)gridDim.x * blockDim.x) {
        const double* a = left + (size_t)il[p] * ld;
        const double* b = right + (size_t)ir[p] * ld;
        double acc = 0.0;
        for (int i = 0; i < len; ++i) {
            const double prod = a[i] * b[i];
            acc = acc + prod;
        }
        out[p] = acc;
    }
}

// One factor of tt_bond_scale_kernel: what the reference multiplies or divides an element by for bond index `i` of a vector of `n`
// values.  Multiply: v[i], 1.0 beyond the vector (vidal.rs:476-480).  Guarded divide: v[i] if it is above 1e-15, else 1.0 (:378-382).
__device__ __forceinline__ double bond_factor(const double* v, int n, int op, int i)
{
    if (i >= n) return 1.0;
    const double x = v[i];
    if (op == TT_SCALE_DIV_GUARD) return x > 1e-15 ? x : 1.0;
    return x;
}
__device__ __forceinline__ double bond_apply(double val, double f, int op)
{
    if (op == TT_SCALE_MUL) return val * f;
    if (op == TT_SCALE_DIV_GUARD) return val / f;
    return val;
}

// Vidal / inverse arithmetic of a whole train in one launch: a ragged batch over a descriptor table.  An item is TT_SCALE_COLS
// passes of 256 / lt columns of one core (lt lanes along l, a power of two; a column is one (s, r) pair, l elements contiguous in
// memory), so consecutive lanes read consecutive doubles and the right-bond factor is read once per column.  Every element is
// dst = (src op_l lv[l]) op_r rv[r]: at most two correctly rounded operations, left factor first (vidal.rs:611-616).
// lop == TT_SCALE_INVERT: the element itself is mapped to 1/v if |v| > 1e-15 else 0 (vidal.rs:648-656), no vectors.
__global__ void __launch_bounds__(256) tt_bond_scale_kernel(const TtScaleDesc* descs, int n_descs, unsigned long long n_items)
{
    const int tid = threadIdx.x;
    for (unsigned long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        // the descriptor this item belongs to: first_item ascends, the last one with first_item <= item
        int lo = 0, hi = n_descs - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (descs[mid].first_item <= item) lo = mid;
            else hi = mid - 1;
        }
        const TtScaleDesc d = descs[lo];
        const int lt = d.lanes, cpp = 256 / lt; // columns per pass
        const int tx = tid & (lt - 1), ty = tid / lt;
        const size_t ncols = (size_t)d.s * d.r;
        const size_t c0 = (size_t)(item - d.first_item) * (size_t)(cpp * TT_SCALE_COLS);
        for (int pass = 0; pass < TT_SCALE_COLS; ++pass) {
            const size_t c = c0 + (size_t)pass * cpp + ty;
            if (c >= ncols) break;
            const int ri = (int)(c / (size_t)d.s);
            const double fr = d.rop == TT_SCALE_NONE ? 1.0 : bond_factor(d.rv, d.rn, d.rop, ri);
            const double* src = d.src + (size_t)d.l * c;
            double* dst = d.dst + (size_t)d.l * c;
            for (int li = tx; li < d.l; li += lt) {
                double val = src[li];
                if (d.lop == TT_SCALE_INVERT) {
                    val = fabs(val) > 1e-15 ? 1.0 / val : 0.0;
                } else {
                    if (d.lop != TT_SCALE_NONE) val = bond_apply(val, bond_factor(d.lv, d.ln, d.lop, li), d.lop);
                    val = bond_apply(val, fr, d.rop);
                }
                dst[li] = val;
            }
        }
    }
}

// out (m x n, ldo) = in (m x n, ldi) * diag(s): one multiply per element (U * S of vidal.rs:106-111), s read once per column
__global__ void __launch_bounds__(256) col_scale_kernel(const double* in, int ldi, int m, int n, const double* __restrict__ s, double* out,
                                                        int ldo)
{
    for (int j = blockIdx.y; j < n; j += gridDim.y) {
        const double f = s[j];
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
            out[i + (size_t)ldo * j] = in[i + (size_t)ldi * j] * f;
    }
}

struct PermuteArgs {
    int rank;
    unsigned long long total;
    unsigned long long out_dims[PERMUTE_MAX_RANK];
    unsigned long long src_stride[PERMUTE_MAX_RANK]; // stride in the input of output axis k
};

__global__ void __launch_bounds__(256) permute_kernel(const double* __restrict__ in, double* __restrict__ out, PermuteArgs a)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < a.total; e += stride) {
        unsigned long long rem = e, src = 0;
        for (int k = 0; k < a.rank; ++k) {
            const unsigned long long d = a.out_dims[k];
            const unsigned long long q = rem / d;
            src += (rem - q * d) * a.src_stride[k];
            rem = q;
        }
        out[e] = in[src];
    }
}

} // namespace

void permute_launch(const double* in, const size_t* dims, const size_t* perm, int rank, double* out, hipStream_t stream)
{
    size_t total = 1;
    for (int k = 0; k < rank; ++k) total *= dims[k];
    if (total == 0) return;
    unsigned long long in_stride[PERMUTE_MAX_RANK];
    for (int k = 0; k < rank; ++k) in_stride[k] = k ? in_stride[k - 1] * dims[k - 1] : 1;
    PermuteArgs a{};
    a.rank = rank;
    a.total = total;
    for (int k = 0; k < rank; ++k) {
        a.out_dims[k] = dims[perm[k]];
        a.src_stride[k] = in_stride[perm[k]];
    }
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(permute_kernel, dim3(blocks), dim3(256), 0, stream, in, out, a);
}

int tt_scale_lanes(int l)
{
    int lt = 1;
    while (lt < l && lt < 256) lt <<= 1;
    return lt;
}

unsigned long long tt_scale_items(int l, int s, int r)
{
    const unsigned long long ncols = (unsigned long long)s * r;
    const unsigned long long per = (unsigned long long)(256 / tt_scale_lanes(l)) * TT_SCALE_COLS;
    return l > 0 ? (ncols + per - 1) / per : 0;
}

void tt_bond_scale_launch(const TtScaleDesc* d_descs, int n_descs, unsigned long long n_items, hipStream_t stream)
{
    if (n_descs <= 0 || n_items == 0) return;
    const unsigned blocks = (unsigned)std::min<unsigned long long>(n_items, TT_SCALE_MAX_BLOCKS);
    hipLaunchKernelGGL(tt_bond_scale_kernel, dim3(blocks), dim3(256), 0, stream, d_descs, n_descs, n_items);
}

void col_scale_launch(const double* in, int ldi, int m, int n, const double* d_s, double* out, int ldo, hipStream_t stream)
{
    if (m <= 0 || n <= 0) return;
    const unsigned bx = (unsigned)std::min((m + 255) / 256, 1024);
    const unsigned by = (unsigned)std::min(n, 1024);
    hipLaunchKernelGGL(col_scale_kernel, dim3(bx, by), dim3(256), 0, stream, in, ldi, m, n, d_s, out, ldo);
}

void core_reshape_launch(const double* in, int L, int S, int R, int mode, double* out, hipStream_t stream)
{
    const size_t total = (size_t)L * S * R;
    if (total == 0) return;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(core_reshape_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, in, L, S, R, mode, out);
}

void tt_sum_launch(const TtCoreDesc* d_cores, int n_sites, int max_bond, double* d_out, hipStream_t stream)
{
    const size_t lds = (size_t)2 * (max_bond > 0 ? max_bond : 1) * 8;
    hipLaunchKernelGGL(tt_sum_kernel, dim3(1), dim3(256), lds, stream, d_cores, n_sites, max_bond, d_out);
}

void tt_norm2_step_launch(const TtCoreDesc& core, const double* d_cur, bool first, double* d_nxt, hipStream_t stream)
{
    const size_t total = (size_t)core.r * core.r;
    if (total == 0) return;
    size_t blocks = (total + 255) / 256;
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(tt_norm2_step_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, core, d_cur, first ? 1 : 0,
                       d_nxt);
}

void tt_env_left_launch(const TtCoreDesc* d_cores, int split, int max_bond, const uint32_t* d_idx, int n_items,
                        double* d_out, int ld, hipStream_t stream)
{
    if (n_items <= 0) return;
    const int blocks = n_items < 8192 ? n_items : 8192;
    const size_t lds = (size_t)2 * (max_bond > 0 ? max_bond : 1) * 8;
    hipLaunchKernelGGL(tt_env_left_kernel, dim3(blocks), dim3(256), lds, stream, d_cores, split, max_bond, d_idx,
                       n_items, d_out, ld);
}

void tt_env_right_launch(const TtCoreDesc* d_cores, int n_sites, int split, int max_bond, const uint32_t* d_idx,
                         int n_items, double* d_out, int ld, hipStream_t stream)
{
    if (n_items <= 0) return;
    const int blocks = n_items < 8192 ? n_items : 8192;
    const size_t lds = (size_t)2 * (max_bond > 0 ? max_bond : 1) * 8;
    hipLaunchKernelGGL(tt_env_right_kernel, dim3(blocks), dim3(256), lds, stream, d_cores, n_sites, split, max_bond,
                       d_idx, n_items, d_out, ld);
}

void tt_env_dot_launch(const double* d_left, const double* d_right, int len, int ld, const uint32_t* d_il,
                       const uint32_t* d_ir, size_t n_pts, double* d_out, hipStream_t stream)
{
    if (n_pts == 0) return;
    size_t blocks = (n_pts + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(tt_env_dot_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_left, d_right, len, ld, d_il,
                       d_ir, n_pts, d_out);
}

} // namespace t4a
