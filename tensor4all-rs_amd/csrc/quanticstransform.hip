// quanticstransform.hip — see quanticstransform.hpp.  Everything up to qt_upload is host integer arithmetic; the difference
// kernel is the naive MPO site contraction of kernels_mpo.hip (mpo_contract, one launch for all sites).
#include "quanticstransform.hpp"

#include <climits>
#include <map>
#include <string>

namespace t4a {

namespace {

[[noreturn]] void invalid(const std::string& msg) { throw Error(T4A_GPU_INVALID_ARGUMENT, msg); }

void check_bc(BoundaryCondition bc)
{
    if ((int)bc < 0 || (int)bc > 2) invalid("unknown boundary condition");
}

double bc_value(BoundaryCondition bc)
{
    return bc == BoundaryCondition::Periodic ? 1.0 : bc == BoundaryCondition::AntiPeriodic ? -1.0 : 0.0;
}

// appends a zero site tensor [l, s1, s2, r] and returns it
std::vector<double>& add_site(QtOperator& op, size_t l, size_t s1, size_t s2, size_t r)
{
    op.dims.push_back({l, s1, s2, r});
    op.sites.emplace_back(l * s1 * s2 * r, 0.0);
    return op.sites.back();
}

// element (l, o, i, r) of a binary site tensor with left bond L
inline size_t at2(size_t L, size_t l, size_t o, size_t i, size_t r) { return l + L * (o + 2 * (i + 2 * r)); }

int64_t add_checked(int64_t x, int64_t y)
{
    int64_t z;
    if (__builtin_add_overflow(x, y, &z)) invalid("affine operator: a carry of A x + b overflows int64");
    return z;
}
int64_t sub_checked(int64_t x, int64_t y)
{
    int64_t z;
    if (__builtin_sub_overflow(x, y, &z)) invalid("affine operator: a carry of A x + b overflows int64");
    return z;
}

} // namespace

// ------------------------------------------------------------------------------------------------ shift
QtOperator qt_shift(size_t r, int64_t offset, BoundaryCondition bc)
{
    check_bc(bc);
    if (r == 0) invalid("Number of sites must be positive");
    if (r > 63) invalid("Number of sites must be at most 63 to avoid integer overflow");
    if (bc == BoundaryCondition::Open && offset < 0) { // shift.rs:136-142
        if (offset == INT64_MIN) invalid("open-boundary shift offset overflow");
        return qt_transpose(qt_shift(r, -offset, bc));
    }
    // offset = nbc * 2^r + offset_mod with 0 <= offset_mod < 2^r
    const __int128 n_max = (__int128)1 << r;
    __int128 offset_mod = (__int128)offset % n_max;
    if (offset_mod < 0) offset_mod += n_max;
    const __int128 nbc = ((__int128)offset - offset_mod) / n_max;
    const uint64_t om = (uint64_t)offset_mod;
    const double bcv = bc_value(bc);

    QtOperator op;
    for (size_t s = 0; s < r; ++s) {
        const size_t y_bit = (om >> (r - 1 - s)) & 1;
        const bool msb = s == 0, lsb = s == r - 1;
        // left = carry out (towards the most significant bit), right = carry in; the boundary weight sits on the carry out of site 0
        const size_t L = msb ? 1 : 2, R = lsb ? 1 : 2;
        std::vector<double>& t = add_site(op, L, 2, 2, R);
        for (size_t cin = 0; cin < R; ++cin)
            for (size_t x = 0; x < 2; ++x) {
                const size_t sum = x + y_bit + cin, out = sum & 1, cout = sum >> 1;
                if (msb) t[at2(L, 0, out, x, cin)] = cout ? bcv : 1.0;
                else t[at2(L, cout, out, x, cin)] = 1.0;
            }
    }
    if (nbc != 0) { // full cycles (shift.rs:266-288)
        double f = 1.0;
        if (bc == BoundaryCondition::AntiPeriodic) f = (nbc % 2 == 0) ? 1.0 : -1.0;
        else if (bc == BoundaryCondition::Open) f = 0.0; // offset >= 2^r here: negative offsets took the transposed branch
        for (double& v : op.sites.back()) v *= f;
    }
    return op;
}

// ------------------------------------------------------------------------------------------------ flip
QtOperator qt_flip(size_t r, BoundaryCondition bc)
{
    check_bc(bc);
    if (r == 0) invalid("Number of sites must be positive");
    if (r == 1) invalid("MPO with one tensor is not supported for flip operator");
    const double bcv = bc_value(bc);
    // 2^r - x bit by bit: out = -a + carry with carry in {-1, 0} (bond index 0 = carry -1, 1 = carry 0); the least
    // significant site starts from carry 0, the carry out of site 0 is 0 only for x = 0, which takes the boundary weight
    QtOperator op;
    for (size_t s = 0; s < r; ++s) {
        const bool msb = s == 0, lsb = s == r - 1;
        const size_t L = msb ? 1 : 2, R = lsb ? 1 : 2;
        std::vector<double>& t = add_site(op, L, 2, 2, R);
        for (size_t c = 0; c < R; ++c) {
            const int carry = lsb ? 0 : (c == 0 ? -1 : 0);
            for (int a = 0; a < 2; ++a) {
                const int out = -a + carry;
                const size_t cout = out < 0 ? 0 : 1, b = (size_t)(out & 1);
                if (msb) t[at2(L, 0, b, a, c)] += cout == 0 ? 1.0 : bcv;
                else t[at2(L, cout, b, a, c)] = 1.0;
            }
        }
    }
    return op;
}

// ------------------------------------------------------------------------------------------------ triangle / cumsum
QtOperator qt_triangle(size_t r, TriangleType triangle)
{
    if ((int)triangle < 0 || (int)triangle > 1) invalid("unknown triangle type");
    if (r < 2) invalid("Number of sites must be at least 2, got " + std::to_string(r));
    // state 0: every bit so far equal; state 1: decided (y > x for Lower, y < x for Upper) at a more significant bit.
    // w[cin][cout][y][x] (cumsum.rs:301-346)
    double w[2][2][2][2] = {};
    w[0][0][0][0] = w[0][0][1][1] = 1.0;
    if (triangle == TriangleType::Lower) w[0][1][1][0] = 1.0;
    else w[0][1][0][1] = 1.0;
    for (int y = 0; y < 2; ++y)
        for (int x = 0; x < 2; ++x) w[1][1][y][x] = 1.0;
    QtOperator op;
    for (size_t s = 0; s < r; ++s) {
        const bool first = s == 0, last = s == r - 1;
        const size_t L = first ? 1 : 2, R = last ? 1 : 2;
        std::vector<double>& t = add_site(op, L, 2, 2, R);
        for (size_t cin = 0; cin < L; ++cin)
            for (size_t y = 0; y < 2; ++y)
                for (size_t x = 0; x < 2; ++x) {
                    if (last) t[at2(L, cin, y, x, 0)] = w[cin][1][y][x]; // only the decided state counts
                    else
                        for (size_t cout = 0; cout < 2; ++cout) t[at2(L, cin, y, x, cout)] = w[cin][cout][y][x];
                }
    }
    return op;
}

// ------------------------------------------------------------------------------------------------ several variables
QtOperator qt_embed(const QtOperator& op, size_t nvariables, size_t target_var)
{
    if (nvariables < 2) invalid("nvariables must be at least 2, got " + std::to_string(nvariables));
    if (target_var >= nvariables)
        invalid("target_var " + std::to_string(target_var) + " must be less than nvariables " + std::to_string(nvariables));
    if (2 * nvariables > 15) // the fused site index 4^nvariables must stay below the tensor train's 65535 (mpo_validate_dims)
        invalid("nvariables " + std::to_string(nvariables) + " is too large: the fused site dimension 4^nvariables exceeds 65535");
    const size_t D = (size_t)1 << nvariables, mask = ~((size_t)1 << target_var) & (D - 1);
    QtOperator e;
    for (size_t s = 0; s < op.len(); ++s) {
        const size_t L = op.dims[s][0], R = op.dims[s][3];
        if (op.dims[s][1] != 2 || op.dims[s][2] != 2) invalid("Input MPO must have binary sites (single variable)");
        const std::vector<double>& src = op.sites[s];
        std::vector<double>& t = add_site(e, L, D, D, R);
        for (size_t o = 0; o < D; ++o)
            for (size_t i = 0; i < D; ++i) {
                if ((o & mask) != (i & mask)) continue; // identity on the other variables
                const size_t ob = (o >> target_var) & 1, ib = (i >> target_var) & 1;
                for (size_t rr = 0; rr < R; ++rr)
                    for (size_t l = 0; l < L; ++l) t[l + L * (o + D * (i + D * rr))] = src[at2(L, l, ob, ib, rr)];
            }
    }
    return e;
}

QtOperator qt_transpose(const QtOperator& op)
{
    QtOperator tr;
    for (size_t s = 0; s < op.len(); ++s) {
        const size_t L = op.dims[s][0], S1 = op.dims[s][1], S2 = op.dims[s][2], R = op.dims[s][3];
        const std::vector<double>& src = op.sites[s];
        std::vector<double>& t = add_site(tr, L, S2, S1, R);
        for (size_t rr = 0; rr < R; ++rr)
            for (size_t j = 0; j < S2; ++j)
                for (size_t i = 0; i < S1; ++i)
                    for (size_t l = 0; l < L; ++l) t[l + L * (j + S2 * (i + S1 * rr))] = src[l + L * (i + S1 * (j + S2 * rr))];
    }
    return tr;
}

// ------------------------------------------------------------------------------------------------ affine
namespace {

using Carry = std::vector<int64_t>;

// AffineCoreData (affine.rs:1631-1639): the carries a site can send on, ascending, and the transitions
// t[(cout * n_in + cin) * site_dim + site] with site = y_bits | x_bits << m
struct AffineCore {
    std::vector<Carry> carries_out;
    std::vector<uint8_t> t;
    size_t n_in = 0, site_dim = 0;
    bool get(size_t cout, size_t cin, size_t site) const { return t[(cout * n_in + cin) * site_dim + site] != 0; }
};

// affine_transform_core (affine.rs:1673-1834): 2 * carry_out = A x + b_curr - scale * y + carry_in, bit by bit
AffineCore affine_core(const std::vector<int64_t>& a, const Carry& b_curr, int64_t scale, size_t m, size_t n,
                       const std::vector<Carry>& carries_in, bool active)
{
    const size_t x_range = active ? (size_t)1 << n : 1, y_range = active ? (size_t)1 << m : 1;
    const size_t site_dim = x_range * y_range, n_in = carries_in.size();
    const bool odd_scale = (scale & 1) != 0;
    std::map<Carry, std::vector<uint8_t>> out; // ordered lexicographically: the bond index of a carry is reproducible (:1807)
    auto record = [&](const Carry& c, size_t cin, size_t site) {
        auto it = out.find(c);
        if (it == out.end()) {
            if ((out.size() + 1) * n_in > (size_t)INT_MAX / site_dim) invalid("affine operator: a site tensor holds more than INT_MAX elements");
            it = out.emplace(c, std::vector<uint8_t>(n_in * site_dim, 0)).first;
        }
        it->second[cin * site_dim + site] = 1;
    };
    Carry z(m), c(m);
    for (size_t ci = 0; ci < n_in; ++ci) {
        const Carry& cin = carries_in[ci];
        for (size_t x = 0; x < x_range; ++x) {
            bool any_odd = false;
            for (size_t i = 0; i < m; ++i) {
                z[i] = add_checked(cin[i], b_curr[i]);
                for (size_t j = 0; j < n; ++j)
                    if ((x >> j) & 1) z[i] = add_checked(z[i], a[i + m * j]);
                any_odd = any_odd || (z[i] & 1);
            }
            if (odd_scale) {
                // one y fits: its bits are the parities of z; an inactive (extension) bit has y = 0
                if (!active && any_odd) continue;
                size_t y = 0;
                for (size_t i = 0; i < m; ++i) {
                    c[i] = z[i];
                    if (z[i] & 1) {
                        y |= (size_t)1 << i;
                        c[i] = sub_checked(c[i], scale);
                    }
                    c[i] >>= 1; // exact: even by construction
                }
                record(c, ci, y | (x << m));
            } else {
                if (any_odd) continue; // scale * y is even: no y fits
                for (size_t y = 0; y < y_range; ++y) {
                    for (size_t i = 0; i < m; ++i) {
                        c[i] = z[i];
                        if ((y >> i) & 1) c[i] = sub_checked(c[i], scale);
                        c[i] >>= 1;
                    }
                    record(c, ci, y | (x << m));
                }
            }
        }
    }
    AffineCore core;
    core.n_in = n_in;
    core.site_dim = site_dim;
    core.t.reserve(out.size() * n_in * site_dim);
    for (auto& kv : out) {
        core.carries_out.push_back(kv.first);
        core.t.insert(core.t.end(), kv.second.begin(), kv.second.end());
    }
    return core;
}

// affine_boundary_weight (affine.rs:531-553)
double boundary_weight(const Carry& carry, const std::vector<BoundaryCondition>& bc)
{
    double w = 1.0;
    for (size_t i = 0; i < carry.size(); ++i) {
        if (bc[i] == BoundaryCondition::AntiPeriodic) w *= (carry[i] & 1) ? -1.0 : 1.0;
        else if (bc[i] == BoundaryCondition::Open) w *= carry[i] == 0 ? 1.0 : 0.0;
    }
    return w;
}

} // namespace

QtOperator qt_affine(size_t r, const std::vector<int64_t>& a, const std::vector<int64_t>& b, int64_t scale, size_t m, size_t n,
                     const std::vector<BoundaryCondition>& bc)
{
    if (m == 0 || n == 0) invalid("affine operator needs at least one output and one input variable");
    if (m > 15 || n > 15 || m + n > 15)
        invalid("affine operator: m + n = " + std::to_string(m + n) + " exceeds 15 (the fused site dimension 2^(m+n) must stay below 65536)");
    if (a.size() != m * n)
        invalid("Matrix A has " + std::to_string(a.size()) + " elements but expected " + std::to_string(m) + "×" + std::to_string(n) + "=" +
                std::to_string(m * n));
    if (b.size() != m) invalid("Vector b has " + std::to_string(b.size()) + " elements but expected " + std::to_string(m));
    if (r == 0) invalid("Number of bits must be positive");
    if (bc.size() != m)
        invalid("Boundary conditions length " + std::to_string(bc.size()) + " doesn't match output dimensions " + std::to_string(m));
    for (BoundaryCondition c : bc) check_bc(c);
    if (scale <= 0) invalid("affine operator: the common denominator must be positive");

    // sign and magnitude of b, so that shifting right ends at zero
    std::vector<int> bsign(m);
    std::vector<uint64_t> b_work(m);
    for (size_t i = 0; i < m; ++i) {
        bsign[i] = b[i] < 0 ? -1 : 1;
        b_work[i] = b[i] < 0 ? (uint64_t)0 - (uint64_t)b[i] : (uint64_t)b[i];
    }
    auto current_bits = [&] {
        Carry bits(m);
        for (size_t i = 0; i < m; ++i) bits[i] = (b_work[i] & 1) ? bsign[i] : 0;
        return bits;
    };
    auto shift_right = [&] {
        for (uint64_t& v : b_work) v >>= 1;
    };

    // carries walk from the least significant bit (site r-1) to site 0: cores[k] belongs to site r-1-k
    std::vector<AffineCore> cores;
    cores.reserve(r);
    const std::vector<Carry> initial{Carry(m, 0)};
    for (size_t k = 0; k < r; ++k) {
        cores.push_back(affine_core(a, current_bits(), scale, m, n, k ? cores.back().carries_out : initial, true));
        shift_right();
    }

    // |b| >= 2^r: the bits of b above the train add sign * (|b| >> r) to every carry out of site 0, and the boundary weight is
    // that of the sum.  For Open this is what the reference's extension loop computes (affine.rs:1445-1523: halving the carry
    // through the remaining bits with x = y = 0 is exact and ends at zero exactly when the sum is zero); for AntiPeriodic the
    // loop drops every odd bit of b, which contradicts affine_transform_matrix (a shift by 2^r must be minus the identity), so
    // the sum's parity is used.  Periodic ignores the carry.
    const AffineCore& top = cores.back();
    std::vector<double> cap(top.carries_out.size());
    for (size_t c = 0; c < cap.size(); ++c) {
        Carry full = top.carries_out[c];
        for (size_t i = 0; i < m; ++i) {
            const int64_t high = (int64_t)b_work[i]; // r >= 1: at most 2^62
            full[i] = add_checked(full[i], bsign[i] < 0 ? -high : high);
        }
        cap[c] = boundary_weight(full, bc);
    }

    QtOperator op;
    const size_t S1 = (size_t)1 << m, S2 = (size_t)1 << n, site_dim = S1 * S2;
    for (size_t s = 0; s < r; ++s) {
        const AffineCore& core = cores[r - 1 - s];
        const bool msb = s == 0, lsb = s == r - 1;
        const size_t n_out = core.carries_out.size();
        const size_t L = msb ? 1 : n_out, R = lsb ? 1 : core.n_in; // at the least significant site n_in is 1 already
        std::vector<double>& t = add_site(op, L, S1, S2, R);
        for (size_t cout = 0; cout < n_out; ++cout) {
            const double w = msb ? cap[cout] : 1.0;
            for (size_t cin = 0; cin < R; ++cin)
                for (size_t site = 0; site < site_dim; ++site) {
                    if (!core.get(cout, cin, site)) continue;
                    // site = y | x << m is the column-major (s1 = y, s2 = x) pair already
                    if (msb) t[site + site_dim * cin] += w;
                    else t[cout + L * (site + site_dim * cin)] = 1.0;
                }
        }
    }
    return op;
}

// ------------------------------------------------------------------------------------------------ device side
std::unique_ptr<Mpo> qt_upload(const QtOperator& op)
{
    mpo_validate_dims(op.dims);
    require_device();
    std::vector<double> flat;
    for (const auto& s : op.sites) flat.insert(flat.end(), s.begin(), s.end());
    if (flat.empty()) flat.push_back(0.0);
    return std::make_unique<Mpo>(op.dims, flat.data());
}

std::unique_ptr<Mpo> qt_difference_kernel(TensorTrain& f, BoundaryCondition bc)
{
    check_bc(bc);
    const size_t r = f.len();
    if (r == 0) invalid("difference kernel requires a non-empty QTT");
    if (bc == BoundaryCondition::Open) invalid("Open boundary is not supported for difference kernels");
    for (size_t s = 0; s < r; ++s)
        if (f.cores[s].s != 2)
            invalid("difference kernel requires binary QTT cores; site " + std::to_string(s) + " has site_dim=" + std::to_string(f.cores[s].s));
    // delta[z; x, x'] = [z = x - x'] is the affine operator z = x - x' (one output, two inputs).  Transposed it is an MPO site
    // [dl, s1 = x + 2 x', k = z, dr]; against f's core read as [fl, k = z, t = 1, fr] the naive site contraction sums z away:
    //   out[dl * f_left + fl, x + 2 x', 0, dr * f_right + fr] = sum_z delta[dl, z, (x, x'), dr] f[fl, z, fr]
    // and the fused x + 2 x' is the column-major (s1, s2) = (x, x') pair of the result.
    const QtOperator delta = qt_transpose(qt_affine(r, {1, -1}, {0}, 1, 1, 2, {bc}));
    require_device();
    std::unique_ptr<Mpo> d = qt_upload(delta);
    std::vector<std::array<size_t, 2>> state_dims(r, {2, 1}), pair_dims(r, {2, 2});
    Mpo state(f.cores, f.eng.stream(), state_dims);
    std::unique_ptr<Mpo> out = mpo_contract(*d, state, MpoAlgorithm::Naive, false, MpoContractionOptions{});
    out->relabel_site_dims(pair_dims);
    return out;
}

} // namespace t4a
