// The per-word arithmetic of the clip's supersampling combine (k_supersample_combine_clip, clip_combine.hip): one
// RGBA8 pixel is one 32-bit word, and the combine's per-byte (l1[c] + l1[c+1] + 2*l2[c] + l3[c] + l3[c+1]) / 6 is done on
// the word's even and odd bytes spread into the 16-bit halves of two words.  Plain C++, so that the host compiles the
// same text (tests/test_clip_supersample_api.py runs it against the per-byte formula).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MM_SS_FN __host__ __device__ inline
#else
#define MM_SS_FN inline
#endif

// Bytes 0 and 2 (e) and bytes 1 and 3 (o) of words, each in a 16-bit half: sums of up to 6 * 255 = 1530 fit a half.
struct mm_ss_halves { uint32_t e, o; };

MM_SS_FN uint32_t mm_ss_even(uint32_t w) { return w & 0x00ff00ffu; }
MM_SS_FN uint32_t mm_ss_odd(uint32_t w) { return (w >> 8) & 0x00ff00ffu; }

// l[c] + l[c+1] of two neighbouring texels of a long row, per channel (at most 510 per half)
MM_SS_FN mm_ss_halves mm_ss_pair_sum(uint32_t left, uint32_t right) {
    mm_ss_halves s;
    s.e = mm_ss_even(left) + mm_ss_even(right);
    s.o = mm_ss_odd(left) + mm_ss_odd(right);
    return s;
}

// v / 6 for every v in 0 .. 1530 (the largest sum); 1530 * 10923 stays below 2^24
MM_SS_FN uint32_t mm_ss_div6(uint32_t v) { return (v * 10923u) >> 16; }

// both halves of a word divided by 6, each quotient (at most 255) left in its half
MM_SS_FN uint32_t mm_ss_div6_halves(uint32_t x) { return mm_ss_div6(x & 0xffffu) | (mm_ss_div6(x >> 16) << 16); }

// One output pixel: `top` and `bottom` are the pair sums of long rows r and r + 1 at the pixel's column, `mid` is the
// short row's texel.
MM_SS_FN uint32_t mm_ss_combine_word(mm_ss_halves top, mm_ss_halves bottom, uint32_t mid) {
    const uint32_t e = top.e + bottom.e + 2u * mm_ss_even(mid);
    const uint32_t o = top.o + bottom.o + 2u * mm_ss_odd(mid);
    return mm_ss_div6_halves(e) | (mm_ss_div6_halves(o) << 8);
}
