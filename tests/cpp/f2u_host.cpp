// f2u_host.cpp -- rt_math.h's f2u_wrap (pack_rgb8's and the texture lookups' float -> uint
// conversion) against the reference's conversion (uint32)(int64)f with its NaN / range guard, on
// the CPU, under the sanitizers: no value may reach an out-of-range conversion.  Exits non-zero
// with a message on the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_math.h"

static uint32_t reference(float f) {
    if (!(f == f) || f >= 9.2e18f || f <= -9.2e18f) return 0u;
    return (uint32_t)(long long)f;
}
static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
static int checked = 0;
static void check(float f) {
    const uint32_t want = reference(f), got = rt::f2u_wrap(f);
    if (got != want) {
        std::printf("f2u_wrap(%a = bits %08x): got %08x, reference %08x\n", f, bits(f), got, want);
        std::exit(1);
    }
    // for 0 <= f < 2^31 the wrap is the plain truncating conversion (what a fast path would use)
    if (f >= 0.0f && f < 2147483648.0f && got != (uint32_t)f) {
        std::printf("f2u_wrap(%a): %08x is not the truncating conversion\n", f, got);
        std::exit(1);
    }
    ++checked;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN(), den = std::numeric_limits<float>::denorm_min();
    std::vector<float> v = {0.0f, -0.0f, 0.999f, 254.999f, 255.0f, 2147483648.0f - 128.0f, 2147483648.0f, 4294967296.0f,
                            4294967296.0f + 1024.0f, -0.5f, -1.0f, -637.5f, -2147483648.0f, -8589934592.0f, inf, -inf,
                            nan, -nan, from_bits(0x7fa00000u), den, -den, from_bits(0x007fffffu), from_bits(0x807fffffu),
                            std::numeric_limits<float>::min()};
    for (float s : {1.0f, -1.0f}) {   // 9.2e18 (the guard) and its float neighbours, either sign
        const float g = s * 9.2e18f;
        v.push_back(g);
        v.push_back(std::nextafterf(g, 0.0f));
        v.push_back(std::nextafterf(std::nextafterf(g, 0.0f), 0.0f));
        v.push_back(std::nextafterf(g, s * inf));
        v.push_back(std::nextafterf(std::nextafterf(g, s * inf), s * inf));
    }
    for (float f : v) check(f);
    if (rt::f2u_wrap(-637.5f) != 0xfffffd83u || rt::f2u_wrap(254.999f) != 254u || rt::f2u_wrap(-0.5f) != 0u ||
        rt::f2u_wrap(4294967296.0f + 1024.0f) != 1024u || rt::f2u_wrap(2147483648.0f) != 0x80000000u ||
        rt::f2u_wrap(nan) != 0u || rt::f2u_wrap(inf) != 0u || rt::f2u_wrap(-9.2e18f) != 0u) {
        std::printf("f2u_wrap: a known value is wrong\n");
        return 1;
    }
    uint32_t s = 0x9e3779b9u;   // 10^6 random bit patterns (xorshift32)
    for (int i = 0; i < 1000000; ++i) {
        s ^= s << 13; s ^= s >> 17; s ^= s << 5;
        check(from_bits(s));
    }
    std::printf("f2u_host ok (%d values)\n", checked);
    return 0;
}
