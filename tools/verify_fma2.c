/* The identity behind the fused doubling of pair-mode loops (hipgen_pair.cpp plan_fusion):
 *     fl(fl(a * 2^k) + b) == fma(a, 2^k, b)   for k = 1, 2, 3 (and a + a for k = 1)   whenever |b| <= 2^102,
 * bit for bit, NaN counted equal to NaN.  Compares the two forms on random bit patterns and on directed inputs (a at the
 * top exponents, denormal a, zeros, infinities, NaN, |b| at 2^102 and one ulp either side, b across the top exponents)
 * and prints, for the inputs inside and outside the guard, how many there were and how many differed.  Outside the guard
 * differences must exist (a * 2^k overflows, the exact sum does not), or the check would prove nothing.
 *
 *     gcc -O2 -ffp-contract=off -march=native tools/verify_fma2.c -o verify_fma2 -lm && ./verify_fma2 [random inputs, default 1e8]
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static int same(float p, float q) { return (p != p && q != q) || u_of(p) == u_of(q); }

static uint64_t n_in, bad_in, n_out, bad_out;
static volatile float sink;

static void check(float a, float b) {
    static const float K[3] = {2.0f, 4.0f, 8.0f};
    const int inside = fabsf(b) <= 0x1p102f;      /* the kernel's guard: NaN fails */
    int bad = 0;
    for (int i = 0; i < 3; ++i) {
        const float d = a * K[i];
        bad += !same(d + b, fmaf(a, K[i], b));
    }
    const float d = a + a;
    bad += !same(d + b, fmaf(a, 2.0f, b));
    if (inside) { n_in += 1; bad_in += bad != 0; }
    else { n_out += 1; bad_out += bad != 0; }
}

static uint64_t rng = 0x9e3779b97f4a7c15ull;
static uint64_t next(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

int main(int argc, char **argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], 0, 10) : 100000000ull;
    /* random bit patterns: half of them as they come, a quarter with a at exponents 0xfd - 0xff, an eighth with a at the top
       finite exponents and b across exponents 0xe0 - 0xfe, an eighth with denormal a */
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t r = next();
        uint32_t a = (uint32_t)r, b = (uint32_t)(r >> 32);
        switch (i & 7) {
            case 0: case 1: a = (a & 0x807fffffu) | ((0xfdu + a % 3u) << 23); break;
            case 2: a = (a & 0x807fffffu) | ((0xfcu + (a >> 8) % 3u) << 23); b = (b & 0x807fffffu) | ((0xe0u + (b >> 8) % 31u) << 23); break;
            case 3: a &= 0x807fffffu; break;
            default: break;
        }
        check(f_of(a), f_of(b));
    }
    /* directed: every pair of the special values */
    uint32_t as[64], bs[64];
    int na = 0, nb = 0;
    for (uint32_t sign = 0; sign < 2; ++sign) {
        const uint32_t s = sign << 31;
        const uint32_t av[] = {0u, 1u, 0x007fffffu, 0x00400000u, 0x00800000u, 0x3f800000u, 0x7e800000u, 0x7effffffu, 0x7f000000u,
                               0x7f7fffffu, 0x7f400000u, 0x7f800000u, 0x7fc00000u, 0x7e000000u, 0x7d800000u, 0x7dffffffu};
        const uint32_t g = 0x72800000u;      /* 2^102 */
        const uint32_t bv[] = {0u, 1u, 0x00800000u, 0x3f800000u, g, g - 1u, g + 1u, 0x73000000u, 0x73800000u, 0x74000000u,
                               0x7f7fffffu, 0x7f800000u, 0x7fc00000u, 0x73ffffffu, 0x7e800000u, 0x7f000000u};
        for (size_t i = 0; i < sizeof av / 4; ++i) as[na++] = av[i] | s;
        for (size_t i = 0; i < sizeof bv / 4; ++i) bs[nb++] = bv[i] | s;
    }
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) check(f_of(as[i]), f_of(bs[j]));
    printf("inside %llu mismatches %llu outside %llu mismatches %llu\n", (unsigned long long)n_in, (unsigned long long)bad_in,
           (unsigned long long)n_out, (unsigned long long)bad_out);
    return bad_in != 0 || bad_out == 0;
}
