// OpenMP CPU backend of bincount (the GPU-less path of csrc/hip/bincount.hip,
// same rules): out[b] = number of elements of x[0, n) equal to b, 0 <= b <
// nbins, int64 counts. Elements are uint8, int32 or int64 at element
// alignment; an element outside [0, nbins) is not counted, and the range test
// is made on the element widened to 64 bits (an int64 2^32 + 3 is out of range
// for nbins = 8).
//
// Where threads x nbins counters are affordable (no more than the input, or a
// small fixed budget) every thread counts its slice of the input into a
// private table and the tables are merged in bin order. Above that the bin
// range is partitioned over the threads and each thread scans the whole input
// for its own bins: no atomics either way, and the counts are exact.
#include <omp.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "cme213/cpu_common.h"

namespace {

using ll = long long;
using ull = unsigned long long;

constexpr ll kPrivateBudget = 1 << 22;  // counters over all threads that are always affordable

// path: 0 by the rule below, 1 serial, 2 private tables, 3 partitioned bins
template <typename T>
void bincount_impl(const T* x, ll n, ll nbins, ll* out, int path) {
    const int threads = omp_get_max_threads();
    if (path == 1 || (path == 0 && (threads <= 1 || n < 4096))) {
        std::memset(out, 0, (size_t)nbins * sizeof(ll));
        for (ll i = 0; i < n; ++i) {
            const ull v = (ull)(ll)x[i];
            if (v < (ull)nbins) ++out[v];
        }
        return;
    }
    const ll all = (ll)threads * nbins;
    if (path == 2 || (path == 0 && (all <= kPrivateBudget || all <= n))) {
        std::vector<ll> priv((size_t)all, 0);
        int used = 1;
#pragma omp parallel
        {
            const int t = omp_get_thread_num(), nt = omp_get_num_threads();
#pragma omp single
            used = nt;
            ll* mine = priv.data() + (size_t)t * (size_t)nbins;
            const ll i0 = n * t / nt, i1 = n * (t + 1) / nt;
            for (ll i = i0; i < i1; ++i) {
                const ull v = (ull)(ll)x[i];
                if (v < (ull)nbins) ++mine[v];
            }
#pragma omp barrier
#pragma omp for schedule(static)
            for (ll b = 0; b < nbins; ++b) {
                ll c = 0;
                for (int k = 0; k < used; ++k) c += priv[(size_t)k * (size_t)nbins + (size_t)b];
                out[b] = c;
            }
        }
        return;
    }
#pragma omp parallel
    {
        const int t = omp_get_thread_num(), nt = omp_get_num_threads();
        const ll b0 = nbins / nt * t + (nbins % nt < t ? nbins % nt : t);
        const ll b1 = b0 + nbins / nt + (t < nbins % nt ? 1 : 0);
        std::memset(out + b0, 0, (size_t)(b1 - b0) * sizeof(ll));
        const ull width = (ull)(b1 - b0);
        for (ll i = 0; i < n; ++i) {
            const ull d = (ull)(ll)x[i] - (ull)b0;  // negative or below b0: far above width
            if (d < width) ++out[b0 + (ll)d];
        }
    }
}

}  // namespace

// esize: 1 uint8, 4 int32, 8 int64. out (nbins int64 counts) is overwritten.
// path: 0 the rule (what cme_cpu_bincount runs), 1 / 2 / 3 one form forced (the
// tests and csrc/checks/bincount_check.cpp reach each at small shapes).
CME_CPU_EXPORT int cme_cpu_bincount_path(const void* x, long long n, int esize, long long nbins, long long* out,
                                         int path) {
    if (n < 0 || nbins < 0 || (esize != 1 && esize != 4 && esize != 8) || path < 0 || path > 3) return 1;
    if (nbins == 0) return 0;
    if (!out || (n > 0 && !x)) return 1;
    if (esize == 1) bincount_impl<uint8_t>((const uint8_t*)x, n, nbins, out, path);
    else if (esize == 4) bincount_impl<int32_t>((const int32_t*)x, n, nbins, out, path);
    else bincount_impl<ll>((const ll*)x, n, nbins, out, path);
    return 0;
}

CME_CPU_EXPORT int cme_cpu_bincount(const void* x, long long n, int esize, long long nbins, long long* out) {
    return cme_cpu_bincount_path(x, n, esize, nbins, out, 0);
}
