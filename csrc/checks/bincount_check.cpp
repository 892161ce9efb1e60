// Stand-alone check of cme_cpu_bincount (csrc/cpu/bincount_cpu.cpp) for a
// sanitizer build: every operand and result lives in a heap block of exactly
// its size (the input as bytes, so that a view starting 1 or 3 elements in is
// a block of its own at element alignment only), so a read or write past an
// end is caught, and every result is compared with a serial loop. The rule
// and each of the three forms (serial, per-thread tables, partitioned bins)
// run on every case. Build and run, from the repository root (one command
// line, then the program):
//
//   g++ -std=c++17 -O1 -g -fopenmp -ffp-contract=off -fsanitize=address,undefined
//       -fno-sanitize-recover=all -Icsrc/include
//       csrc/checks/bincount_check.cpp csrc/cpu/bincount_cpu.cpp -o bincount_check
//   OMP_NUM_THREADS=7 ./bincount_check
//
// Exit status 0 and "ok" on success. Not part of the libraries.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

extern "C" int cme_cpu_bincount(const void* x, long long n, int esize, long long nbins, long long* out);
extern "C" int cme_cpu_bincount_path(const void* x, long long n, int esize, long long nbins, long long* out, int path);

namespace {

using ll = long long;
int failures = 0;

template <typename T>
T draw(std::mt19937_64& rng, ll nbins, int style) {
    const ll lim[] = {(ll)std::numeric_limits<T>::min(), (ll)std::numeric_limits<T>::max(), -1, nbins, nbins - 1, 0,
                      (ll)(1ull << 32) + 3, -(ll)(1ull << 32) + 3};
    ll v;
    if (style == 0) v = (ll)(rng() % (unsigned long long)(nbins + 7)) - 3;  // around the range
    else if (style == 1) v = nbins / 2;                                       // one value: every thread on one bin
    else v = lim[rng() % 8];
    return (T)v;  // narrowing wraps, as the stored element does
}

// Two operands with the same n elements: `x` starts `skew` elements into a
// block that ends at its last element (a misaligned start: malloc's blocks are
// 16-byte aligned), `exact` is a block of exactly n elements.
template <typename T>
void run(ll n, ll nbins, int skew, unsigned seed) {
    std::mt19937_64 rng(seed);
    const size_t bytes = (size_t)n * sizeof(T), lead = (size_t)skew * sizeof(T);
    unsigned char* block = (unsigned char*)std::malloc(lead + bytes ? lead + bytes : 1);
    T* x = reinterpret_cast<T*>(block + lead);
    for (ll i = 0; i < n; ++i) {
        const T v = draw<T>(rng, nbins, (int)((i / 64) % 3));
        std::memcpy(x + i, &v, sizeof(T));
    }
    unsigned char* exact = (unsigned char*)std::malloc(bytes ? bytes : 1);
    std::memcpy(exact, x, bytes);
    std::vector<ll> want((size_t)nbins, 0);
    for (ll i = 0; i < n; ++i) {
        T v;
        std::memcpy(&v, exact + (size_t)i * sizeof(T), sizeof(T));
        const ll w = (ll)v;
        if (w >= 0 && w < nbins) ++want[(size_t)w];
    }
    for (int path = 0; path <= 3; ++path)
        for (int where = 0; where < 2; ++where) {
            const void* src = where ? (const void*)x : (const void*)exact;
            std::vector<ll> out((size_t)nbins, -77);  // overwritten, not accumulated into
            const int rc = path ? cme_cpu_bincount_path(src, n, (int)sizeof(T), nbins, out.data(), path)
                                : cme_cpu_bincount(src, n, (int)sizeof(T), nbins, out.data());
            if (rc != 0 || out != want) {
                std::printf("esize %d n %lld nbins %lld skew %d path %d: rc %d, wrong counts\n", (int)sizeof(T), n,
                            nbins, skew, path, rc);
                ++failures;
            }
        }
    std::free(exact);
    std::free(block);
}

template <typename T>
void shapes() {
    const ll N[] = {0, 1, 2, 15, 16, 17, 255, 4095, 4096, 4097, 20011};
    const ll K[] = {0, 1, 2, 5, 255, 256, 257, 1000, 70001};
    unsigned seed = 1;
    for (ll n : N)
        for (ll k : K)
            for (int skew : {0, 1, 3}) run<T>(n, k, skew, seed++);
}

}  // namespace

int main() {
    shapes<uint8_t>();
    shapes<int32_t>();
    shapes<ll>();
    // refused arguments write nothing
    ll one = 5;
    if (cme_cpu_bincount(nullptr, 1, 4, 1, &one) == 0 || one != 5) ++failures;
    if (cme_cpu_bincount(&one, 1, 2, 1, &one) == 0 || one != 5) ++failures;
    if (cme_cpu_bincount(&one, -1, 8, 1, &one) == 0 || one != 5) ++failures;
    if (cme_cpu_bincount(&one, 1, 8, -1, &one) == 0 || one != 5) ++failures;
    if (cme_cpu_bincount(&one, 1, 8, 1, nullptr) == 0) ++failures;
    if (cme_cpu_bincount_path(&one, 1, 8, 1, &one, 4) == 0 || one != 5) ++failures;
    if (cme_cpu_bincount(nullptr, 0, 8, 0, nullptr) != 0) ++failures;  // nothing to count, nothing to write
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
