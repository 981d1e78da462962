// tt_chain.hpp — the vocabulary of the chain algorithms: a site tensor on the device (DevCore), copies of a chain, the
// Householder-QR sweeps, the two-site split after a truncated SVD, the absorption of an rrLU factor into the neighbouring
// site, and the small host read-back.  Tensor trains, MPOs, the gauge forms, the TCI2 conversion, patching, the fit contraction
// and the linear solver are all written against it.  Host code only: every launch goes to the stream it is given.
#pragma once

#include <algorithm>
#include <vector>

#include "engine.hpp"

namespace t4a {

// One site tensor in HBM, a column-major (left, site, right) block.
struct DevCore {
    DevBuf<double> buf;
    size_t l = 0, s = 0, r = 0;
    size_t size() const { return l * s * r; }
    // Sets the shape on the existing buffer: no reallocation when the capacity suffices, so a pointer a chain kernel holds stays good.
    void reshape(size_t l_, size_t s_, size_t r_)
    {
        l = l_;
        s = s_;
        r = r_;
        buf.reserve(std::max<size_t>(size(), 1));
    }
    static DevCore make(size_t l, size_t s, size_t r)
    {
        DevCore c;
        c.reshape(l, s, r);
        return c;
    }
};

// Device-to-device copies queued on `st`; an empty core copies nothing.
DevCore clone_core(const DevCore& src, hipStream_t st);
std::vector<DevCore> clone_cores(const std::vector<DevCore>& src, hipStream_t st);

// A buffer that may still be read on the stream is not handed back to the pool before the stream has drained: the sync happens
// only when the buffer really has to grow.
inline void grow(Engine& e, DevBuf<double>& b, size_t n)
{
    n = std::max<size_t>(n, 1);
    if (n <= b.cap) return;
    e.sync();
    b.reserve(n);
}

// `count` values of a device vector in a fresh host vector: async copy plus sync, nothing for count == 0.
std::vector<double> to_host(Engine& eng, const double* d_src, size_t count);

// QR sweeps with the thin Householder QR (right_canonicalize, canonical.rs:35-89).  right_step: site i becomes Q^T of its transposed
// l x (s r) matricisation (k = min(l, s r) rows) and R^T goes into its left neighbour; left_step: site i becomes Q of its (l s) x r
// matricisation and R goes into its right neighbour.  Each step ends synced, since it releases the two old cores.
// A step is its factorising half followed by the absorbing GEMM.  The factorising halves, for callers that do something of their own
// with the triangular factor (the bond correction of one-site TDVP): factor_left -> Q as the core (l, s, k) and R (k x r) in rr;
// factor_right -> Q^T as the core (k, s, r) and R (k x l, its transpose is the factor to the left of Q^T) in rr.  They sync nothing and
// leave `c` as it is; rr holds the factor until the next step of this sweep.
struct QrSweep {
    Engine& eng;
    hipStream_t st;
    DevBuf<double> m1, q, rr;
    explicit QrSweep(Engine& e) : eng(e), st(e.stream()) {}
    DevCore factor_right(const DevCore& c);
    DevCore factor_left(const DevCore& c);
    void right_step(std::vector<DevCore>& cores, size_t i);
    void left_step(std::vector<DevCore>& cores, size_t i);
    // sites < center from the left, then sites > center from the right
    void canonicalize(std::vector<DevCore>& cores, size_t center);
};

// The two sites of a truncated SVD theta (M x N) = U (M x k, ldU) diag(S) Vt (k x N, ldVt) with `keep` values kept, written into
// `left` (keep columns) and `right` (keep rows), whose shapes the caller has set.  Moving right: left = U, right = diag(S) Vt;
// moving left: left = U diag(S), right = Vt.
void split_two_site(hipStream_t st, const double* U, int ldU, const double* S, const double* Vt, int ldVt, int N, int keep, bool move_right,
                    DevCore& left, DevCore& right);

// The rrLU sweeps (TensorTrain::compress, TensorCI2::from_tensor_train), after a factorisation left eng.left() (M x rk) and
// eng.right() (rk x N) behind.  The left factor of an (L S) x R bond matrix as the core (L, S, rk); the right factor of an L x (S R)
// bond matrix as the core (rk, S, R).
DevCore core_from_left_factor(Engine& eng, size_t L, size_t S, size_t rk);
DevCore core_from_right_factor(Engine& eng, size_t rk, size_t S, size_t R);
// next <- eng.right() (rk x next.l) * next, prev <- prev * eng.left() (prev.r x rk): reshape into m1, GEMM into m2, reshape into
// the new core that is returned.  Nothing is synced: the caller does that before it releases the old core.
DevCore absorb_right_into_next(Engine& eng, size_t rk, const DevCore& next, DevBuf<double>& m1, DevBuf<double>& m2);
DevCore absorb_left_into_prev(Engine& eng, size_t rk, const DevCore& prev, DevBuf<double>& m1, DevBuf<double>& m2);

} // namespace t4a
