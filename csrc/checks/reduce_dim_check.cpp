// Stand-alone check of cme_cpu_reduce_dim (csrc/cpu/reduce_dim_cpu.cpp) for a
// sanitizer build: every operand and result lives in a heap block of exactly
// its size, so a read or write past an end is caught, and every result is
// compared with a serial statement of the rules. Build and run, from the
// repository root (one command line, then the program):
//
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined
//       -fno-sanitize-recover=all -Icsrc/include
//       csrc/checks/reduce_dim_check.cpp csrc/cpu/reduce_dim_cpu.cpp -o reduce_dim_check
//   OMP_NUM_THREADS=7 ./reduce_dim_check
//
// Exit status 0 and "ok" on success. Not part of the libraries.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <type_traits>
#include <vector>

extern "C" int cme_cpu_reduce_dim(const void* in, void* out, void* out_indices, long long outer, long long n,
                                  long long inner, int dtype, int op);

namespace {

using ll = long long;
int failures = 0;

template <typename T> bool is_nan(T v) { return v != v; }

template <typename T> bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// S: the unsigned type sums wrap in
template <typename T, typename S>
void run(int dtype, ll outer, ll n, ll inner, unsigned seed) {
    std::mt19937_64 rng(seed);
    const size_t size = (size_t)(outer * n * inner), lines = (size_t)(outer * inner);
    std::vector<T> x(size);
    constexpr bool fl = std::is_floating_point<T>::value;
    for (size_t k = 0; k < size; ++k) {
        const int r = (int)(rng() % 23);
        if (fl && r == 0) x[k] = (T)std::numeric_limits<double>::quiet_NaN();
        else if (fl && r == 1) x[k] = (T)-0.0;
        else if (r == 2) x[k] = (T)0;
        else x[k] = (T)((ll)(rng() % 17) - 8);
        if ((k / (size_t)inner / (size_t)n) % 3 == 1 && fl && is_nan(x[k])) x[k] = (T)3;  // some slabs without NaN
    }
    for (int op = 0; op < 3; ++op) {
        for (int pair = 0; pair < 2; ++pair) {
            if (pair && op == 0) continue;
            std::vector<T> out(lines);
            std::vector<ll> idx(pair ? lines : 0);
            const int rc = cme_cpu_reduce_dim(x.data(), out.data(), pair ? idx.data() : nullptr, outer, n, inner, dtype, op);
            if (rc != 0) {
                std::printf("rc %d: dtype %d op %d pair %d (%lld, %lld, %lld)\n", rc, dtype, op, pair, outer, n, inner);
                ++failures;
                continue;
            }
            for (ll o = 0; o < outer; ++o)
                for (ll j = 0; j < inner; ++j) {
                    auto at = [&](ll i) { return x[(size_t)((o * n + i) * inner + j)]; };
                    const T got = out[(size_t)(o * inner + j)];
                    bool ok;
                    if (op == 0) {
                        if (fl) {
                            double s = 0;  // small integers, NaN aside: exact in any order
                            for (ll i = 0; i < n; ++i) s += (double)at(i);
                            ok = is_nan(s) ? is_nan(got) : (double)got == s;
                        } else {
                            S s = 0;
                            for (ll i = 0; i < n; ++i) s += (S)at(i);
                            ok = (S)got == s;
                        }
                    } else {
                        // first NaN, else the first element equal to the extreme
                        ll w = 0;
                        for (ll i = 1; i < n && !is_nan(at(w)); ++i)
                            if (is_nan(at(i)) || (op == 1 ? at(i) > at(w) : at(i) < at(w))) w = i;
                        if (pair) {
                            ok = idx[(size_t)(o * inner + j)] == w && same_bits(got, at(w));
                        } else if (is_nan(at(w))) {
                            ok = is_nan(got);
                        } else {
                            // of zeros of both signs, max is +0.0 and min is -0.0
                            T want = at(w);
                            if (fl && want == (T)0)
                                for (ll i = 0; i < n; ++i)
                                    if (at(i) == (T)0 && std::signbit((double)at(i)) == (op == 2)) want = at(i);
                            ok = same_bits(got, want);
                        }
                    }
                    if (!ok) {
                        if (failures < 20)
                            std::printf("mismatch: dtype %d op %d pair %d (%lld, %lld, %lld) line (%lld, %lld)\n", dtype, op,
                                        pair, outer, n, inner, o, j);
                        ++failures;
                    }
                }
        }
    }
}

}  // namespace

int main() {
    // n == 1, around the unroll depth and the tile stand-ins, odd sizes; inner
    // around the column block of 512; few lines (chunks along n, the last one
    // short or empty) and many
    const ll shapes[][3] = {{1, 1, 1},    {1, 2, 1},    {1, 5, 1},     {1, 4097, 1}, {3, 1, 1},   {3, 7, 1},   {3, 1025, 1},
                            {67, 257, 1}, {1027, 65, 1}, {1, 1, 3},    {1, 9, 3},    {3, 8, 5},   {3, 129, 64}, {2, 7, 511},
                            {2, 9, 512},  {1, 129, 513}, {1, 3, 1025}, {1, 2, 2},    {5, 100, 4}, {1, 1000, 2}, {40, 8, 1}};
    unsigned seed = 1;
    for (const auto& s : shapes) {
        run<float, float>(0, s[0], s[1], s[2], seed++);
        run<int32_t, uint32_t>(1, s[0], s[1], s[2], seed++);
        run<uint32_t, uint32_t>(2, s[0], s[1], s[2], seed++);
        run<int64_t, uint64_t>(3, s[0], s[1], s[2], seed++);
        run<double, double>(4, s[0], s[1], s[2], seed++);
    }
    // refused arguments and empty operands touch nothing
    float one = 1.0f, res = 0.0f;
    ll where = -1;
    if (cme_cpu_reduce_dim(&one, &res, &where, 1, 1, 1, 0, 0) == 0) ++failures;  // a sum has no index
    if (cme_cpu_reduce_dim(&one, &res, nullptr, 1, 1, 1, 7, 0) == 0) ++failures;  // no such dtype
    if (cme_cpu_reduce_dim(&one, &res, nullptr, 1, 0, 1, 0, 1) != 0 || res != 0.0f) ++failures;
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
