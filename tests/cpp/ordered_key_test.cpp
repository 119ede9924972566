// The order-preserving map double <-> uint64 of the ingest kernels' extrema (kinematic_icp_amd/csrc/kicp_ordered_key.hpp), the
// header's own two functions on the CPU, over the value set of the numpy re-enactment in tests/test_ingest.py: normal values of
// both signs, subnormals, the zeros, the infinities, epoch stamps in seconds and nanoseconds.  Checked: a < b  =>  key(a) < key(b)
// (on the values sorted as doubles: monotone), key(a) == key(b) only for equal bit patterns, -0.0 below +0.0, the infinities at
// the ends, ordered_value(ordered_key(v)) == v bit for bit, and the smallest / largest key map back to the smallest / largest value
// - what k_ingest's fold relies on.  Stand-alone (own main), built with -fsanitize=address,undefined by tests/test_ordered_key.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "kicp_ordered_key.hpp"

using kicp::ordered_key;
using kicp::ordered_value;

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), tiny = std::numeric_limits<double>::denorm_min();
    std::mt19937_64 rng(21);
    std::normal_distribution<double> wide(0.0, 1e9), small(0.0, 1e-300), velodyne(-0.05, 0.03);
    std::vector<double> v;
    for (int i = 0; i < 5000; ++i) v.push_back(wide(rng));
    for (int i = 0; i < 100; ++i) v.push_back(small(rng));
    for (int i = 0; i < 1000; ++i) v.push_back(velodyne(rng));
    for (double s : {0.0, -0.0, tiny, -tiny, inf, -inf, 1.7e9, 1.7e18, -0.1, 9999999999.4, 1e10 * 1e-9, 4294967295.0,
                     std::numeric_limits<double>::max(), std::numeric_limits<double>::lowest(), std::numeric_limits<double>::min()})
        v.push_back(s);
    // the inverse, bit for bit - and the keys of the two zeros differ
    for (double x : v) CHECK(bits(ordered_value(ordered_key(x))) == bits(x));
    CHECK(ordered_key(-0.0) < ordered_key(0.0));
    CHECK(ordered_key(-0.0) + 1 == ordered_key(0.0));  // (nothing sorts between them)
    CHECK(ordered_key(-tiny) < ordered_key(-0.0) && ordered_key(0.0) < ordered_key(tiny));
    // monotone: sorted as doubles (the zeros by sign), the keys rise strictly wherever the bit patterns differ
    std::sort(v.begin(), v.end(), [](double a, double b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); });
    for (size_t i = 1; i < v.size(); ++i) {
        const unsigned long long a = ordered_key(v[i - 1]), b = ordered_key(v[i]);
        CHECK(bits(v[i - 1]) == bits(v[i]) ? a == b : a < b);
    }
    // the infinities at the ends of every finite value; the fold's neutral elements (~0 for the minimum, 0 for the maximum) beyond them
    CHECK(v.front() == -inf && v.back() == inf);
    for (double x : v) CHECK(ordered_key(-inf) <= ordered_key(x) && ordered_key(x) <= ordered_key(inf));
    CHECK(ordered_key(inf) < ~0ull && ordered_key(-inf) > 0ull);
    // what the last workgroup hands the host: the smallest and the largest key are the smallest and the largest value
    unsigned long long kmin = ~0ull, kmax = 0ull;
    for (double x : v) kmin = std::min(kmin, ordered_key(x)), kmax = std::max(kmax, ordered_key(x));
    CHECK(ordered_value(kmin) == -inf && ordered_value(kmax) == inf);
    std::vector<double> finite(v.begin() + 1, v.end() - 1);
    kmin = ~0ull, kmax = 0ull;
    for (double x : finite) kmin = std::min(kmin, ordered_key(x)), kmax = std::max(kmax, ordered_key(x));
    CHECK(bits(ordered_value(kmin)) == bits(finite.front()) && bits(ordered_value(kmax)) == bits(finite.back()));
    std::printf("OK\n");
    return 0;
}
