// Stand-alone check of cme_cpu_sort_dim (csrc/cpu/sort_dim_cpu.cpp) for a
// sanitizer build: every operand and result lives in a heap block of exactly
// its size, so a read or write past an end is caught, and every result is
// compared with a serial statement of the rules (an insertion sort under a
// comparison written out per type, not through order codes). Build and run,
// from the repository root (one command line, then the program):
//
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined
//       -fno-sanitize-recover=all -Icsrc/include
//       csrc/checks/sort_dim_check.cpp csrc/cpu/sort_dim_cpu.cpp -o sort_dim_check
//   OMP_NUM_THREADS=7 ./sort_dim_check
//
// Exit status 0 and "ok" on success. Not part of the libraries.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <type_traits>
#include <vector>

extern "C" int cme_cpu_sort_dim(const void* in, void* out_values, void* out_indices, long long outer, long long n,
                                long long inner, int dtype, int descending);

namespace {

using ll = long long;
int failures = 0;

template <typename T> bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// a strictly before b in ascending order. Integers: their natural order.
// Floats: IEEE total order -- a NaN with the sign bit set below everything, a
// NaN without it above everything, NaNs of one sign by their payload bits
// (away from zero), -0.0 below +0.0, everything else numerically.
template <typename T>
bool before(T a, T b) {
    if constexpr (std::is_floating_point<T>::value) {
        using U = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
        U x, y;
        std::memcpy(&x, &a, sizeof(T));
        std::memcpy(&y, &b, sizeof(T));
        const bool na = a != a, nb = b != b, sa = (x >> (sizeof(T) * 8 - 1)) != 0, sb = (y >> (sizeof(T) * 8 - 1)) != 0;
        if (na || nb || (a == 0 && b == 0)) {
            if (sa != sb) return sa;              // the negative one first
            if (na && nb) return sa ? x > y : x < y;
            if (na) return sa;                    // -NaN before a number, +NaN after
            if (nb) return !sb;
            return false;                         // zeros of one sign
        }
        return a < b;
    } else {
        return a < b;
    }
}

template <typename T>
T draw(std::mt19937_64& rng, int style) {
    using U = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
    constexpr U sign = (U)1 << (sizeof(U) * 8 - 1);
    // the keys whose order code is all ones or all zeros in either direction, then small keys
    const U edge[] = {(U)~(U)0, (U)0, sign, (U)~sign};
    const int r = (int)(rng() % 16);
    U bits;
    if (style == 0) bits = (U)rng();  // any bit pattern: NaNs of both signs, payloads, infinities
    else if (style == 1) bits = (U)(rng() % 4) * (U)0x9e3779b97f4a7c15ull;  // four keys: heavy ties
    else bits = r < 4 ? edge[r] : (U)(rng() % 7);
    T v;
    std::memcpy(&v, &bits, sizeof(T));
    return v;
}

template <typename T>
void run(int dtype, ll outer, ll n, ll inner, unsigned seed) {
    std::mt19937_64 rng(seed);
    const size_t size = (size_t)(outer * n * inner);
    std::vector<T> x(size);
    for (size_t k = 0; k < size; ++k) x[k] = draw<T>(rng, (int)((k / (size_t)(n > 0 ? n : 1)) % 3));
    for (int desc = 0; desc < 2; ++desc) {
        std::vector<T> val(size);
        std::vector<ll> idx(size);
        const int rc = cme_cpu_sort_dim(x.data(), val.data(), idx.data(), outer, n, inner, dtype, desc);
        if (rc != 0) {
            std::printf("rc %d: dtype %d desc %d (%lld, %lld, %lld)\n", rc, dtype, desc, outer, n, inner);
            ++failures;
            continue;
        }
        for (ll o = 0; o < outer; ++o)
            for (ll j = 0; j < inner; ++j) {
                auto at = [&](ll i) { return (size_t)((o * n + i) * inner + j); };
                std::vector<ll> want((size_t)n);
                for (ll i = 0; i < n; ++i) {  // stable insertion: move left past strictly later keys only
                    ll p = i;
                    while (p > 0 && (desc ? before(x[at(want[(size_t)p - 1])], x[at(i)])
                                          : before(x[at(i)], x[at(want[(size_t)p - 1])]))) {
                        want[(size_t)p] = want[(size_t)p - 1];
                        --p;
                    }
                    want[(size_t)p] = i;
                }
                for (ll i = 0; i < n; ++i) {
                    if (idx[at(i)] != want[(size_t)i] || !same_bits(val[at(i)], x[at(want[(size_t)i])])) {
                        std::printf("dtype %d desc %d (%lld, %lld, %lld) line (%lld, %lld) position %lld: index %lld, "
                                    "expected %lld\n", dtype, desc, outer, n, inner, o, j, i, idx[at(i)], want[(size_t)i]);
                        ++failures;
                        break;
                    }
                }
            }
    }
}

template <typename T>
void shapes(int dtype) {
    const ll S[][3] = {{1, 1, 1}, {1, 257, 1}, {7, 33, 1}, {1, 40, 9}, {3, 17, 5}, {5, 1, 4}, {2, 64, 3},
                       {0, 5, 2}, {2, 0, 3}, {2, 5, 0}, {40, 2, 1}, {1, 2, 40}};
    unsigned seed = 1;
    for (const auto& s : S) run<T>(dtype, s[0], s[1], s[2], seed++);
}

}  // namespace

int main() {
    shapes<uint32_t>(0);
    shapes<int32_t>(1);
    shapes<float>(2);
    shapes<uint64_t>(3);
    shapes<int64_t>(4);
    shapes<double>(5);
    // refused arguments write nothing
    if (cme_cpu_sort_dim(nullptr, nullptr, nullptr, 1, 1, 1, 0, 0) == 0) ++failures;
    if (cme_cpu_sort_dim(nullptr, nullptr, nullptr, 1, 1, 1, 6, 0) == 0) ++failures;
    if (cme_cpu_sort_dim(nullptr, nullptr, nullptr, -1, 1, 1, 0, 0) == 0) ++failures;
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
