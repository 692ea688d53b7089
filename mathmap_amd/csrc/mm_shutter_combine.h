// The per-pixel arithmetic of the shutter combine (k_shutter_combine_clip, clip_combine.hip; the semantics are stated
// at mmhip_render_clip_shutter in include/mmhip.h): the time of a sub-sample, the sequential f32 sum of a pixel's
// sub-samples, its scale by 1 / K, and the pixel store's byte conversions for output_bpp 1 - 4 (mm_store_pixel in
// mm_device.h: CLAMP01, products in double, truncation).  Plain C++, so that the host compiles the same text
// (tests/test_clip_shutter_api.py runs it against a NumPy restatement).  Compile without floating-point contraction:
// neither the sum nor the grey value may become an fma.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define MM_SHUTTER_FN __attribute__((host)) __attribute__((device)) inline
#else
#define MM_SHUTTER_FN inline
#endif

// The time of sub-sample j of K of a frame at time t: double arithmetic, the product before the quotient, one rounding.
MM_SHUTTER_FN float mm_shutter_sample_t(float t, float span, int j, int k) {
    return (float)((double)t + ((double)span * (double)j) / (double)k);
}

MM_SHUTTER_FN float mm_shutter_inv_k(int k) { return (float)(1.0 / (double)k); }

// one channel: acc + f (f_0 + f_1 + ... in that order), and the mean acc * inv_k
MM_SHUTTER_FN float mm_shutter_add(float acc, float f) { return acc + f; }
MM_SHUTTER_FN float mm_shutter_scale(float acc, float inv_k) { return acc * inv_k; }

// CLAMP01 as the store sees it: NaN and -0 leave byte 0, like 0 does
MM_SHUTTER_FN float mm_shutter_clamp01(float x) { return !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x); }

MM_SHUTTER_FN unsigned char mm_shutter_byte(float c) { return (unsigned char)(int)((double)mm_shutter_clamp01(c) * 255.0); }

MM_SHUTTER_FN unsigned char mm_shutter_grey(float r, float g, float b) {
    const double v = ((double)mm_shutter_clamp01(r) * 0.299 + (double)mm_shutter_clamp01(g) * 0.587 + (double)mm_shutter_clamp01(b) * 0.114) * 255.0;
    return (unsigned char)(int)v;
}

// The pixel store of the mean m (r, g, b, a) at output_bpp `bpp`: grey for 1 and 2, alpha at bpp - 1 for 2 and 4.
MM_SHUTTER_FN void mm_shutter_store_bytes(unsigned char *p, float r, float g, float b, float a, int bpp) {
    if (bpp == 1 || bpp == 2)
        p[0] = mm_shutter_grey(r, g, b);
    else {
        p[0] = mm_shutter_byte(r);
        p[1] = mm_shutter_byte(g);
        p[2] = mm_shutter_byte(b);
    }
    if (bpp == 2 || bpp == 4) p[bpp - 1] = mm_shutter_byte(a);
}
