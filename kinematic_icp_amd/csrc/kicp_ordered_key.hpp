// kicp_ordered_key.hpp -- the order-preserving map double -> uint64 (and back) through which the ingest kernels merge the stamps'
// extrema as integers (kicp_pre_ingest.hpp k_ingest, k_ingest_scan; the host reads the result back with ordered_value, kicp_pre_ingest.hip).
// -0.0 sorts below +0.0, the infinities sit at the ends, NaNs beyond them.  No HIP in here beyond the device's own bit cast, so
// tests/cpp/ordered_key_test.cpp compiles this very file with g++ and checks both functions on the CPU.
#pragma once
#ifndef KICP_HD
#define KICP_HD inline
#endif

namespace kicp {
KICP_HD unsigned long long ordered_key(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
#else
    unsigned long long b;
    __builtin_memcpy(&b, &v, 8);
#endif
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
KICP_HD double ordered_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
}
}  // namespace kicp
