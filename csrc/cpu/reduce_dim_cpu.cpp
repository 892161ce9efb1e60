// OpenMP CPU backend of the reductions along one dimension (the GPU-less path
// of csrc/hip/reduce_dim.hip, same rules): a contiguous tensor seen as (outer,
// n, inner), element (o, i, j) at (o*n + i)*inner + j, line (o, j) reduced
// over i to a value or to a (value, index) pair.
//
//  * sum: in the element type; integers are summed unsigned and wrap.
//  * max / min, values only: IEEE 754-2019 maximum / minimum (a NaN in the
//    line gives NaN, +0.0 is above -0.0).
//  * max / min with indices: the first NaN if the line has one, else the first
//    element equal to the extreme (torch.max(x, dim) on CPU tensors). Pairs
//    join as: the better value wins (NaN beats any non-NaN), on a tie the
//    smaller index; "no candidate" carries the largest int64 as its index.
//
// A work item is a block of up to kColBlock adjacent columns of one `o` (a row
// when inner == 1) and one of K chunks along n; K > 1 where there are fewer
// such lines than threads. The partials of a line are folded in chunk order,
// so a float sum's tree is fixed by the shape and the thread count.
#include <omp.h>

#include <cstdint>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "cme213/cpu_common.h"

namespace {

using ll = long long;
constexpr ll kColBlock = 512;
constexpr ll kNone = std::numeric_limits<ll>::max();

template <typename T>
T lowest() {
    return std::is_floating_point<T>::value ? -std::numeric_limits<T>::infinity() : std::numeric_limits<T>::lowest();
}
template <typename T>
T highest() {
    return std::is_floating_point<T>::value ? std::numeric_limits<T>::infinity() : std::numeric_limits<T>::max();
}

// of two equal floats: AND of the bits is +0.0 if either is, OR is -0.0 if either is
template <typename T, bool kAnd>
T equal_pick(T a, T b) {
    typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type x, y;
    std::memcpy(&x, &a, sizeof(T));
    std::memcpy(&y, &b, sizeof(T));
    x = kAnd ? (x & y) : (x | y);
    std::memcpy(&a, &x, sizeof(T));
    return a;
}

struct Sum {
    static constexpr bool kPair = false;
    template <typename T> static T identity() { return T(0); }
    template <typename T> static T fold(T a, T b) { return a + b; }
};
struct Max {
    static constexpr bool kPair = false;
    template <typename T> static T identity() { return lowest<T>(); }
    template <typename T> static T fold(T a, T b) {
        if (std::is_floating_point<T>::value) {
            if (a != a) return a;
            if (b != b) return b;
            if (a == b) return equal_pick<T, true>(a, b);
        }
        return a > b ? a : b;
    }
};
struct Min {
    static constexpr bool kPair = false;
    template <typename T> static T identity() { return highest<T>(); }
    template <typename T> static T fold(T a, T b) {
        if (std::is_floating_point<T>::value) {
            if (a != a) return a;
            if (b != b) return b;
            if (a == b) return equal_pick<T, false>(a, b);
        }
        return a < b ? a : b;
    }
};
// wins(a, ai, b, bi): the pair b replaces the pair a
struct ArgMax {
    static constexpr bool kPair = true;
    template <typename T> static T identity() { return lowest<T>(); }
    template <typename T> static bool wins(T a, ll ai, T b, ll bi) {
        const bool na = a != a, nb = b != b;
        return (nb && !na) || b > a || ((a == b || (na && nb)) && bi < ai);
    }
};
struct ArgMin {
    static constexpr bool kPair = true;
    template <typename T> static T identity() { return highest<T>(); }
    template <typename T> static bool wins(T a, ll ai, T b, ll bi) {
        const bool na = a != a, nb = b != b;
        return (nb && !na) || b < a || ((a == b || (na && nb)) && bi < ai);
    }
};

template <typename T, typename R>
inline void take(T& v, ll& i, T x, ll xi) {
    if constexpr (R::kPair) {
        if (R::wins(v, i, x, xi)) {
            v = x;
            i = xi;
        }
    } else {
        v = R::fold(v, x);
    }
}

template <typename T, typename R>
void reduce_dim_impl(const T* in, T* out, ll* idx, ll outer, ll n, ll inner) {
    const T id = R::template identity<T>();
    const ll nb = (inner + kColBlock - 1) / kColBlock;
    const ll lines = outer * nb;
    const int nt = omp_get_max_threads();
    ll K = 1;
    if (lines < nt) K = (nt + lines - 1) / lines;
    if (K > n) K = n;
    if (K < 1) K = 1;
    const ll chunk = (n + K - 1) / K;
    std::vector<T> partv;
    std::vector<ll> parti;
    if (K > 1) {
        partv.assign((std::size_t)(outer * K * inner), id);
        if (R::kPair) parti.assign((std::size_t)(outer * K * inner), kNone);
    }
    T* const ov = K > 1 ? partv.data() : out;
    ll* const oi = K > 1 ? parti.data() : idx;
    const ll items = lines * K;
#pragma omp parallel for schedule(static)
    for (ll item = 0; item < items; ++item) {
        const ll b = item % nb, k = (item / nb) % K, o = item / (nb * K);
        const ll j0 = b * kColBlock, w = (j0 + kColBlock < inner ? j0 + kColBlock : inner) - j0;
        const ll i0 = k * chunk < n ? k * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
        T run[kColBlock];
        ll runi[kColBlock];
        for (ll j = 0; j < w; ++j) {
            run[j] = id;
            runi[j] = kNone;
        }
        for (ll i = i0; i < i1; ++i) {
            const T* p = in + (o * n + i) * inner + j0;
            for (ll j = 0; j < w; ++j) take<T, R>(run[j], runi[j], p[j], i);
        }
        const ll at = (o * K + k) * inner + j0;
        for (ll j = 0; j < w; ++j) {
            ov[at + j] = run[j];
            if (R::kPair) oi[at + j] = runi[j];
        }
    }
    if (K == 1) return;
#pragma omp parallel for schedule(static)
    for (ll c = 0; c < outer * inner; ++c) {
        const ll at = (c / inner) * K * inner + c % inner;
        T run = id;
        ll runi = kNone;
        for (ll k = 0; k < K; ++k) take<T, R>(run, runi, partv[at + k * inner], R::kPair ? parti[at + k * inner] : 0);
        out[c] = run;
        if (R::kPair) idx[c] = runi;
    }
}

// S: the unsigned type integer sums wrap in (T itself for the floats)
template <typename T, typename S>
int reduce_dim_dispatch(const void* in, void* out, void* idx, ll outer, ll n, ll inner, int op) {
    if (idx) {
        if (op == 1) reduce_dim_impl<T, ArgMax>((const T*)in, (T*)out, (ll*)idx, outer, n, inner);
        else if (op == 2) reduce_dim_impl<T, ArgMin>((const T*)in, (T*)out, (ll*)idx, outer, n, inner);
        else return 1;
        return 0;
    }
    if (op == 0) reduce_dim_impl<S, Sum>((const S*)in, (S*)out, nullptr, outer, n, inner);
    else if (op == 1) reduce_dim_impl<T, Max>((const T*)in, (T*)out, nullptr, outer, n, inner);
    else if (op == 2) reduce_dim_impl<T, Min>((const T*)in, (T*)out, nullptr, outer, n, inner);
    else return 1;
    return 0;
}

}  // namespace

// Reduction along the middle dimension of a contiguous (outer, n, inner)
// tensor: out holds outer * inner elements, line (o, j) at [o*inner + j].
// out_indices: null for values only, else int64 positions along n (op 1 / 2
// only). dtype: 0 float32, 1 int32, 2 uint32, 3 int64, 4 float64; op: 0 sum,
// 1 max, 2 min. Nothing is written for an empty operand (n == 0 included).
CME_CPU_EXPORT int cme_cpu_reduce_dim(const void* in, void* out, void* out_indices, long long outer, long long n,
                                      long long inner, int dtype, int op) {
    if (outer < 0 || n < 0 || inner < 0 || op < 0 || op > 2 || (out_indices && op == 0)) return 1;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    if (!in || !out) return 1;
    if (dtype == 0) return reduce_dim_dispatch<float, float>(in, out, out_indices, outer, n, inner, op);
    if (dtype == 1) return reduce_dim_dispatch<int32_t, uint32_t>(in, out, out_indices, outer, n, inner, op);
    if (dtype == 2) return reduce_dim_dispatch<uint32_t, uint32_t>(in, out, out_indices, outer, n, inner, op);
    if (dtype == 3) return reduce_dim_dispatch<int64_t, uint64_t>(in, out, out_indices, outer, n, inner, op);
    if (dtype == 4) return reduce_dim_dispatch<double, double>(in, out, out_indices, outer, n, inner, op);
    return 1;
}
