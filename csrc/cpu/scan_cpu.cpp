// OpenMP CPU backends for scans / reductions / segmented scans (oracles and
// GPU-less path). Parallel scan = per-thread block sums, serial scan of the
// sums, per-thread add-back (the CPU analogue of scan-then-add).
#include <omp.h>

#include <cstdint>
#include <limits>
#include <type_traits>
#include <vector>

#include "cme213/cpu_common.h"

namespace {

template <typename T>
void scan_impl(const T* in, T* out, long long n, bool exclusive) {
    int nt = omp_get_max_threads();
    std::vector<T> sums(nt + 1, T(0));
#pragma omp parallel num_threads(nt)
    {
        int t = omp_get_thread_num();
        int tn = omp_get_num_threads();
        long long b = n * t / tn, e = n * (t + 1) / tn;
        T acc = T(0);
        for (long long i = b; i < e; ++i) acc += in[i];
        sums[t + 1] = acc;
#pragma omp barrier
#pragma omp single
        for (int k = 1; k <= tn; ++k) sums[k] += sums[k - 1];
        T run = sums[t];
        for (long long i = b; i < e; ++i) {
            T v = in[i];
            if (exclusive) {
                out[i] = run;
                run += v;
            } else {
                run += v;
                out[i] = run;
            }
        }
    }
}

// Running max / min (torch.cummax / cummin values): a is the earlier operand.
// NaN is sticky and among equal values the later one wins (+0.0 / -0.0), so
// the operators are associative but not commutative.
struct CumMax {
    template <typename T> T operator()(T a, T b) const { return (b >= a || b != b) ? b : a; }
    template <typename T> static T identity() {
        return std::numeric_limits<T>::has_infinity ? -std::numeric_limits<T>::infinity()
                                                    : std::numeric_limits<T>::lowest();
    }
};
struct CumMin {
    template <typename T> T operator()(T a, T b) const { return (b <= a || b != b) ? b : a; }
    template <typename T> static T identity() {
        return std::numeric_limits<T>::has_infinity ? std::numeric_limits<T>::infinity()
                                                    : std::numeric_limits<T>::max();
    }
};

// The three phases of scan_impl for an operator called as op(earlier, later):
// per-thread block totals, their serial exclusive scan in block order, the
// per-thread rescan from the block's carry. out may be in.
template <typename T, typename Op>
void scan_op_impl(const T* in, T* out, long long n, bool exclusive, Op op) {
    const T id = Op::template identity<T>();
    int nt = omp_get_max_threads();
    std::vector<T> sums(nt + 1, id);
#pragma omp parallel num_threads(nt)
    {
        int t = omp_get_thread_num();
        int tn = omp_get_num_threads();
        long long b = n * t / tn, e = n * (t + 1) / tn;
        T acc = id;
        for (long long i = b; i < e; ++i) acc = op(acc, in[i]);
        sums[t + 1] = acc;
#pragma omp barrier
#pragma omp single
        for (int k = 1; k <= tn; ++k) sums[k] = op(sums[k - 1], sums[k]);
        T run = sums[t];
        for (long long i = b; i < e; ++i) {
            T v = in[i];
            if (exclusive) {
                out[i] = run;
                run = op(run, v);
            } else {
                run = op(run, v);
                out[i] = run;
            }
        }
    }
}

template <typename T>
int scan_op_dispatch(const void* in, void* out, long long n, int op, bool exclusive) {
    if (op == 1) scan_op_impl((const T*)in, (T*)out, n, exclusive, CumMax());
    else if (op == 2) scan_op_impl((const T*)in, (T*)out, n, exclusive, CumMin());
    else return 1;
    return 0;
}

template <typename T>
void reduce_impl(const T* in, long long n, int op, T* out) {
    T acc;
    if (op == 0 && sizeof(T) == 8) {
        // 64-bit elements accumulate in their own type: uint64 sums wrap
        // modulo 2^64 (int64 is summed through it), double has no wider oracle
        T a = T(0);
#pragma omp parallel for reduction(+ : a)
        for (long long i = 0; i < n; ++i) a += in[i];
        acc = a;
    } else if (op == 0 && std::is_integral<T>::value) {
        // int32 sums wrap modulo 2^32, as the GPU kernels' do: summed unsigned
        // (a double sum cast back to int is undefined once it leaves the range)
        uint32_t a = 0;
#pragma omp parallel for reduction(+ : a)
        for (long long i = 0; i < n; ++i) a += (uint32_t)in[i];
        acc = (T)a;
    } else if (op == 0) {
        double a = 0;  // fp64 accumulation for the oracle
#pragma omp parallel for reduction(+ : a)
        for (long long i = 0; i < n; ++i) a += (double)in[i];
        acc = (T)a;
    } else if (op == 1) {
        acc = in[0];
#pragma omp parallel for reduction(max : acc)
        for (long long i = 0; i < n; ++i) acc = in[i] > acc ? in[i] : acc;
    } else {
        acc = in[0];
#pragma omp parallel for reduction(min : acc)
        for (long long i = 0; i < n; ++i) acc = in[i] < acc ? in[i] : acc;
    }
    *out = acc;
}

}  // namespace

CME_CPU_EXPORT int cme_cpu_scan(const void* in, void* out, long long n, int dtype, int exclusive) {
    if (dtype == 0) scan_impl((const float*)in, (float*)out, n, exclusive);
    // int32 in unsigned arithmetic too: the sum wraps modulo 2^32
    else if (dtype == 1) scan_impl((const uint32_t*)in, (uint32_t*)out, n, exclusive);
    else if (dtype == 2) scan_impl((const uint32_t*)in, (uint32_t*)out, n, exclusive);
    // int64 in unsigned arithmetic: the sum wraps modulo 2^64 (signed overflow is undefined)
    else if (dtype == 3) scan_impl((const uint64_t*)in, (uint64_t*)out, n, exclusive);
    else if (dtype == 4) scan_impl((const double*)in, (double*)out, n, exclusive);
    else return 1;
    return 0;
}

// op: 0 sum (cme_cpu_scan), 1 max, 2 min -- the running max / min of
// torch.cummax / cummin (values only). dtype as cme_cpu_scan; int64 compares as
// signed.
CME_CPU_EXPORT int cme_cpu_scan_op(const void* in, void* out, long long n, int dtype, int op, int exclusive) {
    if (op == 0) return cme_cpu_scan(in, out, n, dtype, exclusive);
    if (dtype == 0) return scan_op_dispatch<float>(in, out, n, op, exclusive);
    if (dtype == 1) return scan_op_dispatch<int32_t>(in, out, n, op, exclusive);
    if (dtype == 2) return scan_op_dispatch<uint32_t>(in, out, n, op, exclusive);
    if (dtype == 3) return scan_op_dispatch<int64_t>(in, out, n, op, exclusive);
    if (dtype == 4) return scan_op_dispatch<double>(in, out, n, op, exclusive);
    return 1;
}

namespace {

struct Sum {
    template <typename T> T operator()(T a, T b) const { return a + b; }
    template <typename T> static T identity() { return T(0); }
};

// Scan of (outer, n, inner) along n: element (o, i, j) at (o*n + i)*inner + j.
// A work item is a block of up to kColBlock adjacent columns of one `o` (a row
// when inner == 1), walked down i with the running values in a small array.
// Where there are fewer such lines than threads, n is split into K chunks and
// the three phases of scan_op_impl run over (line, chunk) items: totals, their
// serial exclusive scan along the chunks, the rescan from each chunk's carry.
// op is always called as op(earlier, later); out may be in.
constexpr long long kColBlock = 512;

template <typename T, typename Op>
void scan_dim_impl(const T* in, T* out, long long outer, long long n, long long inner, bool exclusive, Op op) {
    const T id = Op::template identity<T>();
    const long long nb = (inner + kColBlock - 1) / kColBlock;
    const long long lines = outer * nb;
    const int nt = omp_get_max_threads();
    long long K = 1;
    if (lines < nt) K = (nt + lines - 1) / lines;
    if (K > n) K = n;
    const long long chunk = (n + K - 1) / K;
    std::vector<T> tot;
    if (K > 1) tot.assign((std::size_t)(outer * K * inner), id);
    auto walk = [&](long long item, bool totals_only) {
        const long long b = item % nb, k = (item / nb) % K, o = item / (nb * K);
        const long long j0 = b * kColBlock, w = (j0 + kColBlock < inner ? j0 + kColBlock : inner) - j0;
        const long long i0 = k * chunk < n ? k * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
        T* t = K > 1 ? tot.data() + (o * K + k) * inner + j0 : nullptr;
        T run[kColBlock];
        for (long long j = 0; j < w; ++j) run[j] = (K > 1 && !totals_only) ? t[j] : id;
        for (long long i = i0; i < i1; ++i) {
            const T* p = in + (o * n + i) * inner + j0;
            T* q = out + (o * n + i) * inner + j0;
            for (long long j = 0; j < w; ++j) {
                const T inc = op(run[j], p[j]);
                if (!totals_only) q[j] = exclusive ? run[j] : inc;
                run[j] = inc;
            }
        }
        if (totals_only)
            for (long long j = 0; j < w; ++j) t[j] = run[j];
    };
    const long long items = lines * K;
    if (K > 1) {
#pragma omp parallel for schedule(static)
        for (long long item = 0; item < items; ++item) walk(item, true);
#pragma omp parallel for schedule(static)
        for (long long c = 0; c < outer * inner; ++c) {
            T* t = tot.data() + (c / inner) * K * inner + c % inner;
            T run = id;
            for (long long k = 0; k < K; ++k) {
                const T v = t[k * inner];
                t[k * inner] = run;
                run = op(run, v);
            }
        }
    }
#pragma omp parallel for schedule(static)
    for (long long item = 0; item < items; ++item) walk(item, false);
}

template <typename T, typename S>
int scan_dim_dispatch(const void* in, void* out, long long outer, long long n, long long inner, int op, bool exclusive) {
    // S: the unsigned type integer sums wrap in (T itself for the floats)
    if (op == 0) scan_dim_impl((const S*)in, (S*)out, outer, n, inner, exclusive, Sum());
    else if (op == 1) scan_dim_impl((const T*)in, (T*)out, outer, n, inner, exclusive, CumMax());
    else if (op == 2) scan_dim_impl((const T*)in, (T*)out, outer, n, inner, exclusive, CumMin());
    else return 1;
    return 0;
}

}  // namespace

// Scan along the middle dimension of a contiguous (outer, n, inner) tensor.
// dtype as cme_cpu_scan, op as cme_cpu_scan_op, the same rules: integer sums
// wrap, max / min are torch.cummax / cummin values.
CME_CPU_EXPORT int cme_cpu_scan_dim(const void* in, void* out, long long outer, long long n, long long inner,
                                    int dtype, int op, int exclusive) {
    if (outer < 0 || n < 0 || inner < 0) return 1;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    if (dtype == 0) return scan_dim_dispatch<float, float>(in, out, outer, n, inner, op, exclusive);
    if (dtype == 1) return scan_dim_dispatch<int32_t, uint32_t>(in, out, outer, n, inner, op, exclusive);
    if (dtype == 2) return scan_dim_dispatch<uint32_t, uint32_t>(in, out, outer, n, inner, op, exclusive);
    if (dtype == 3) return scan_dim_dispatch<int64_t, uint64_t>(in, out, outer, n, inner, op, exclusive);
    if (dtype == 4) return scan_dim_dispatch<double, double>(in, out, outer, n, inner, op, exclusive);
    return 1;
}

namespace {

// Running max / min with the position of the winner (torch.cummax / cummin:
// values and indices). The carry is a pair (v, i), i the position along n or
// -1 for "none"; pairs join with the earlier operand first, and the later one
// replaces it iff it is not none and passes the test of CumMax / CumMin. So a
// later NaN or equal value takes the index, and a real element always beats
// the identity value.
struct ArgMax {
    using Val = CumMax;
    template <typename T> static bool later(T a, T b) { return b >= a || b != b; }
};
struct ArgMin {
    using Val = CumMin;
    template <typename T> static bool later(T a, T b) { return b <= a || b != b; }
};

template <typename A, typename T>
inline void join(T& av, long long& ai, T bv, long long bi) {
    if (bi >= 0 && A::later(av, bv)) {
        av = bv;
        ai = bi;
    }
}

// The three phases of scan_dim_impl over pairs: pair totals of every (line,
// chunk) item, their serial exclusive scan along the chunks, the rescan of
// each chunk from its carry pair. out may be in.
template <typename T, typename A>
void cumarg_dim_impl(const T* in, T* out, long long* idx, long long outer, long long n, long long inner) {
    const T id = A::Val::template identity<T>();
    const long long nb = (inner + kColBlock - 1) / kColBlock;
    const long long lines = outer * nb;
    const int nt = omp_get_max_threads();
    long long K = 1;
    if (lines < nt) K = (nt + lines - 1) / lines;
    if (K > n) K = n;
    const long long chunk = (n + K - 1) / K;
    std::vector<T> totv;
    std::vector<long long> toti;
    if (K > 1) {
        totv.assign((std::size_t)(outer * K * inner), id);
        toti.assign((std::size_t)(outer * K * inner), -1);
    }
    auto walk = [&](long long item, bool totals_only) {
        const long long b = item % nb, k = (item / nb) % K, o = item / (nb * K);
        const long long j0 = b * kColBlock, w = (j0 + kColBlock < inner ? j0 + kColBlock : inner) - j0;
        const long long i0 = k * chunk < n ? k * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
        const long long at = (o * K + k) * inner + j0;
        T run[kColBlock];
        long long runi[kColBlock];
        for (long long j = 0; j < w; ++j) {
            const bool seeded = K > 1 && !totals_only;
            run[j] = seeded ? totv[at + j] : id;
            runi[j] = seeded ? toti[at + j] : -1;
        }
        for (long long i = i0; i < i1; ++i) {
            const long long row = (o * n + i) * inner + j0;
            for (long long j = 0; j < w; ++j) {
                join<A>(run[j], runi[j], in[row + j], i);
                if (!totals_only) {
                    out[row + j] = run[j];
                    idx[row + j] = runi[j];
                }
            }
        }
        if (totals_only)
            for (long long j = 0; j < w; ++j) {
                totv[at + j] = run[j];
                toti[at + j] = runi[j];
            }
    };
    const long long items = lines * K;
    if (K > 1) {
#pragma omp parallel for schedule(static)
        for (long long item = 0; item < items; ++item) walk(item, true);
#pragma omp parallel for schedule(static)
        for (long long c = 0; c < outer * inner; ++c) {
            const long long at = (c / inner) * K * inner + c % inner;
            T run = id;
            long long runi = -1;
            for (long long k = 0; k < K; ++k) {
                const T v = totv[at + k * inner];
                const long long vi = toti[at + k * inner];
                totv[at + k * inner] = run;
                toti[at + k * inner] = runi;
                join<A>(run, runi, v, vi);
            }
        }
    }
#pragma omp parallel for schedule(static)
    for (long long item = 0; item < items; ++item) walk(item, false);
}

template <typename T>
int cumarg_dim_dispatch(const void* in, void* out, void* idx, long long outer, long long n, long long inner, int op) {
    if (op == 1) cumarg_dim_impl<T, ArgMax>((const T*)in, (T*)out, (long long*)idx, outer, n, inner);
    else if (op == 2) cumarg_dim_impl<T, ArgMin>((const T*)in, (T*)out, (long long*)idx, outer, n, inner);
    else return 1;
    return 0;
}

}  // namespace

// Running max (op 1) / min (op 2) along the middle dimension of a contiguous
// (outer, n, inner) tensor with the position of the winner along n: the
// (values, indices) of torch.cummax / cummin. dtype as cme_cpu_scan;
// out_values may be in, out_indices is int64.
CME_CPU_EXPORT int cme_cpu_cumarg_dim(const void* in, void* out_values, void* out_indices, long long outer,
                                      long long n, long long inner, int dtype, int op) {
    if (outer < 0 || n < 0 || inner < 0) return 1;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    if (dtype == 0) return cumarg_dim_dispatch<float>(in, out_values, out_indices, outer, n, inner, op);
    if (dtype == 1) return cumarg_dim_dispatch<int32_t>(in, out_values, out_indices, outer, n, inner, op);
    if (dtype == 2) return cumarg_dim_dispatch<uint32_t>(in, out_values, out_indices, outer, n, inner, op);
    if (dtype == 3) return cumarg_dim_dispatch<int64_t>(in, out_values, out_indices, outer, n, inner, op);
    if (dtype == 4) return cumarg_dim_dispatch<double>(in, out_values, out_indices, outer, n, inner, op);
    return 1;
}

CME_CPU_EXPORT int cme_cpu_reduce(const void* in, long long n, int dtype, int op, void* out) {
    if (n <= 0) return 1;
    if (dtype == 0) reduce_impl((const float*)in, n, op, (float*)out);
    else if (dtype == 1) reduce_impl((const int*)in, n, op, (int*)out);
    else if (dtype == 3 && op == 0) reduce_impl((const uint64_t*)in, n, op, (uint64_t*)out);
    else if (dtype == 3) reduce_impl((const int64_t*)in, n, op, (int64_t*)out);
    else if (dtype == 4) reduce_impl((const double*)in, n, op, (double*)out);
    else return 1;
    return 0;
}

// Sequential inclusive segmented scan (the reference checker's semantics,
// hw/hw_final/programming/aux/reference_spMVscan-released.cu:38-54), with an
// optional fused multiply. Parallelised over segments found from the flags.
CME_CPU_EXPORT int cme_cpu_segscan(const float* in, const float* xmul, float* out, const void* flags, int mode,
                                   long long n) {
    auto head = [&](long long i) -> bool {
        if (mode == 0) return ((const uint8_t*)flags)[i] != 0;
        return (((const uint32_t*)flags)[i >> 5] >> (i & 31)) & 1u;
    };
    std::vector<long long> starts;
    starts.push_back(0);
    for (long long i = 1; i < n; ++i)
        if (head(i)) starts.push_back(i);
    starts.push_back(n);
    long long ns = (long long)starts.size() - 1;
#pragma omp parallel for schedule(dynamic, 64)
    for (long long sgi = 0; sgi < ns; ++sgi) {
        float run = 0.f;
        for (long long i = starts[sgi]; i < starts[sgi + 1]; ++i) {
            float v = xmul ? in[i] * xmul[i] : in[i];
            run = (i == starts[sgi]) ? v : run + v;
            out[i] = run;
        }
    }
    return 0;
}

namespace {

template <typename T>
void segscan64_impl(const T* in, const T* xmul, T* out, const void* flags, int mode, long long n) {
    auto head = [&](long long i) -> bool {
        if (mode == 0) return ((const uint8_t*)flags)[i] != 0;
        return (((const uint32_t*)flags)[i >> 5] >> (i & 31)) & 1u;
    };
    std::vector<long long> starts;
    starts.push_back(0);  // element 0 starts a segment whether or not its flag is set
    for (long long i = 1; i < n; ++i)
        if (head(i)) starts.push_back(i);
    starts.push_back(n);
    const long long ns = (long long)starts.size() - 1;
#pragma omp parallel for schedule(dynamic, 64)
    for (long long sgi = 0; sgi < ns; ++sgi) {
        T run = T(0);
        for (long long i = starts[sgi]; i < starts[sgi + 1]; ++i) {
            const T v = xmul ? in[i] * xmul[i] : in[i];
            run = (i == starts[sgi]) ? v : run + v;
            out[i] = run;
        }
    }
}

}  // namespace

// The same for 8-byte elements: dtype 3 int64 (summed as uint64: wraps modulo
// 2^64), 4 float64. Serial within a segment, parallel across segments; out
// may be in.
CME_CPU_EXPORT int cme_cpu_segscan64(const void* in, const void* xmul, void* out, const void* flags, int mode,
                                     long long n, int dtype) {
    if (n <= 0) return 0;
    if (dtype == 3) segscan64_impl((const uint64_t*)in, (const uint64_t*)xmul, (uint64_t*)out, flags, mode, n);
    else if (dtype == 4) segscan64_impl((const double*)in, (const double*)xmul, (double*)out, flags, mode, n);
    else return 1;
    return 0;
}
