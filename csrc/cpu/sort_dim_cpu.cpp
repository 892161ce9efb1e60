// OpenMP CPU backend of the sort along one dimension (the GPU-less path of
// csrc/hip/sort_dim.hip, same rules): a contiguous tensor seen as (outer, n,
// inner), element (o, i, j) at (o*n + i)*inner + j; every line (o, j) is
// sorted stably over i, and the result is the pair (values, int64 positions
// along n).
//
// Keys are compared through order codes: unsigned integers as they are, signed
// ones with the sign bit flipped, floats in IEEE total order (-NaN < -inf < ...
// < -0 < +0 < ... < +inf < +NaN). Descending order complements the code, so
// equal keys keep their input order in both directions. values is the operand
// gathered at the indices, bit for bit.
//
// A thread takes whole lines: it gathers the line into (code, position)
// pairs, sorts them stably by code and scatters keys and positions. Lines of
// any length; only element alignment is assumed.
#include <omp.h>

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "cme213/cpu_common.h"

namespace {

using ll = long long;

// kind: 0 unsigned, 1 signed, 2 float
template <typename U>
U code_of(U k, int kind, bool descending) {
    constexpr U sign = (U)1 << (sizeof(U) * 8 - 1);
    if (kind == 1) k ^= sign;
    if (kind == 2) k ^= (k & sign) ? ~(U)0 : sign;
    return descending ? (U)~k : k;
}

template <typename U>
void sort_dim_impl(const U* in, U* values, ll* indices, ll outer, ll n, ll inner, int kind, bool descending) {
    const ll lines = outer * inner;
#pragma omp parallel
    {
        std::vector<std::pair<U, ll>> buf((size_t)n);
#pragma omp for schedule(static)
        for (ll c = 0; c < lines; ++c) {
            const ll o = c / inner, j = c % inner;
            const ll at = o * n * inner + j;
            for (ll i = 0; i < n; ++i) buf[(size_t)i] = {code_of(in[at + i * inner], kind, descending), i};
            std::stable_sort(buf.begin(), buf.end(),
                             [](const std::pair<U, ll>& a, const std::pair<U, ll>& b) { return a.first < b.first; });
            for (ll i = 0; i < n; ++i) {
                const ll src = buf[(size_t)i].second;
                values[at + i * inner] = in[at + src * inner];
                indices[at + i * inner] = src;
            }
        }
    }
}

}  // namespace

// Stable sort of a contiguous (outer, n, inner) tensor along n. out_values:
// the sorted lines in the operand's type and layout; out_indices: the int64
// position along n every output element came from. dtype: 0 uint32, 1 int32,
// 2 float32, 3 uint64, 4 int64, 5 float64. Nothing is written for an empty
// operand.
CME_CPU_EXPORT int cme_cpu_sort_dim(const void* in, void* out_values, void* out_indices, long long outer, long long n,
                                    long long inner, int dtype, int descending) {
    if (outer < 0 || n < 0 || inner < 0 || dtype < 0 || dtype > 5) return 1;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    if (!in || !out_values || !out_indices) return 1;
    if (dtype < 3)
        sort_dim_impl<uint32_t>((const uint32_t*)in, (uint32_t*)out_values, (ll*)out_indices, outer, n, inner, dtype % 3,
                                descending != 0);
    else
        sort_dim_impl<uint64_t>((const uint64_t*)in, (uint64_t*)out_values, (ll*)out_indices, outer, n, inner, dtype % 3,
                                descending != 0);
    return 0;
}
