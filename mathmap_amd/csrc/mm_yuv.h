// The arithmetic and the layout of a clip's planar Y'CbCr 4:2:0 output (k_rgba8_to_yuv420_clip, clip_yuv.hip; the
// semantics are stated at mmhip_clip_to_yuv420 in include/mmhip.h): the coefficient tables of the four modes, the luma of
// a pixel, the chroma of a 2 x 2 block, and where the planes of a frame lie.  Plain C++, so that the host compiles the
// same text: the launcher takes a mode's coefficients from the table, both paths of the kernel convert with the two
// formulas, and a stand-alone test program (tests/test_clip_yuv_api.py) runs all of it on a frame worked out by hand.
// All of it is int32; every shift is an arithmetic shift of a signed value (floor division) -- but for the quantiser of the
// 10-bit output and the matrix of the 10-bit input at the end, which are float32 and say so.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define MM_YUV_FN __attribute__((host)) __attribute__((device)) inline
#else
#define MM_YUV_FN inline
#endif

enum { MM_YUV_BT601 = 0, MM_YUV_BT709 = 1, MM_YUV_MATRICES = 2 };
enum { MM_YUV_LIMITED = 0, MM_YUV_FULL = 1, MM_YUV_RANGES = 2 };

// One mode: Y = ((yr R + yg G + yb B + 2^15) >> 16) + off; the chroma rows take the sums of a 2 x 2 block.  Each
// coefficient is floor(k * 2^16 + 0.5) of the standard's constant, but for the green luma coefficient and one chroma
// coefficient per row, which make the row sum exactly: white is 235 or 255, grey has chroma 128.
struct mm_yuv_mode {
    int off;
    int yr, yg, yb;
    int cbr, cbg, cbb;
    int crr, crg, crb;
};

// [matrix][range]
static const mm_yuv_mode MM_YUV_MODES[MM_YUV_MATRICES][MM_YUV_RANGES] = {
    {{16, 16829, 33039, 6416, -9714, -19071, 28785, 28784, -24103, -4681},      // bt601 limited
     {0, 19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329}},     // bt601 full
    {{16, 11966, 40254, 4064, -6596, -22189, 28785, 28784, -26145, -2639},      // bt709 limited
     {0, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005}},      // bt709 full
};

inline bool mm_yuv_mode_known(int matrix, int range) {
    return matrix >= 0 && matrix < MM_YUV_MATRICES && range >= 0 && range < MM_YUV_RANGES;
}

// The luma of one pixel: 16 .. 235 or 0 .. 255 by construction, no clamp.
MM_YUV_FN int mm_yuv_luma(const mm_yuv_mode &m, int r, int g, int b) { return ((m.yr * r + m.yg * g + m.yb * b + (1 << 15)) >> 16) + m.off; }

// One chroma sample from the sums of its block's four pixels and the row's coefficients.  The clamp matters at full
// range only, where pure blue and pure red give 256.
MM_YUV_FN int mm_yuv_chroma(int kr, int kg, int kb, int rs, int gs, int bs) {
    const int c = ((kr * rs + kg * gs + kb * bs + (1 << 17)) >> 18) + 128;
    return c < 0 ? 0 : c > 255 ? 255 : c;
}
MM_YUV_FN int mm_yuv_cb(const mm_yuv_mode &m, int rs, int gs, int bs) { return mm_yuv_chroma(m.cbr, m.cbg, m.cbb, rs, gs, bs); }
MM_YUV_FN int mm_yuv_cr(const mm_yuv_mode &m, int rs, int gs, int bs) { return mm_yuv_chroma(m.crr, m.crg, m.crb, rs, gs, bs); }

// A frame: the Y plane, width * height bytes with rows `width` apart, then Cb, then Cr, each cw * ch bytes with rows cw
// apart.
MM_YUV_FN int mm_yuv_cw(int width) { return (width + 1) >> 1; }
MM_YUV_FN int mm_yuv_ch(int height) { return (height + 1) >> 1; }
MM_YUV_FN int64_t mm_yuv_cb_offset(int width, int height) { return (int64_t)width * height; }
MM_YUV_FN int64_t mm_yuv_cr_offset(int width, int height) { return (int64_t)width * height + (int64_t)mm_yuv_cw(width) * mm_yuv_ch(height); }
MM_YUV_FN int64_t mm_yuv_frame_bytes(int width, int height) { return (int64_t)width * height + 2 * (int64_t)mm_yuv_cw(width) * mm_yuv_ch(height); }

// A whole frame on the host, as the kernel converts it: rgba is height rows of width RGBA8 pixels row_stride bytes apart
// (the alpha byte is not read), dst one frame of mm_yuv_frame_bytes.  An odd last column or row is replicated.
inline void mm_yuv_frame_host(const mm_yuv_mode &m, const unsigned char *rgba, int64_t row_stride, int width, int height, unsigned char *dst) {
    const int cw = mm_yuv_cw(width), ch = mm_yuv_ch(height);
    unsigned char *cb = dst + mm_yuv_cb_offset(width, height), *cr = dst + mm_yuv_cr_offset(width, height);
    for (int r = 0; r < height; ++r)
        for (int c = 0; c < width; ++c) {
            const unsigned char *p = rgba + r * row_stride + (int64_t)c * 4;
            dst[(int64_t)r * width + c] = (unsigned char)mm_yuv_luma(m, p[0], p[1], p[2]);
        }
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            int rs = 0, gs = 0, bs = 0;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const int c = 2 * cx + i < width ? 2 * cx + i : width - 1, r = 2 * cy + j < height ? 2 * cy + j : height - 1;
                    const unsigned char *p = rgba + r * row_stride + (int64_t)c * 4;
                    rs += p[0];
                    gs += p[1];
                    bs += p[2];
                }
            cb[(int64_t)cy * cw + cx] = (unsigned char)mm_yuv_cb(m, rs, gs, bs);
            cr[(int64_t)cy * cw + cx] = (unsigned char)mm_yuv_cr(m, rs, gs, bs);
        }
}

// ---- the other direction: planar Y'CbCr 4:2:0 frames to the drawable's words (k_yuv420_to_rgba_clip, clip_yuv_in.hip;
// the semantics are stated at mmhip_clip_from_yuv420 in include/mmhip.h) ----
enum { MM_YUV_CHROMA_BILINEAR = 0, MM_YUV_CHROMA_REPLICATE = 1, MM_YUV_CHROMAS = 2 };

// One mode: with y = Y - off, u = Cb' - 128, v = Cr' - 128,
//   R = clamp((ky y + rcr v + 2^15) >> 16), G = clamp((ky y + gcb u + gcr v + 2^15) >> 16), B = clamp((ky y + bcb u + 2^15) >> 16).
// Each coefficient is the standard's constant with its magnitude rounded as floor(|k| * 2^16 + 0.5), the sign kept.
struct mm_yuv_rgba_mode {
    int off;
    int ky, rcr, gcb, gcr, bcb;
};

// [matrix][range]
static const mm_yuv_rgba_mode MM_YUV_RGBA_MODES[MM_YUV_MATRICES][MM_YUV_RANGES] = {
    {{16, 76309, 104597, -25675, -53279, 132201},      // bt601 limited
     {0, 65536, 91881, -22553, -46802, 116130}},       // bt601 full
    {{16, 76309, 117489, -13975, -34925, 138438},      // bt709 limited
     {0, 65536, 103206, -12276, -30679, 121609}},      // bt709 full
};

inline bool mm_yuv_chroma_known(int chroma) { return chroma >= 0 && chroma < MM_YUV_CHROMAS; }

MM_YUV_FN int mm_yuv_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// One pixel's drawable word, R << 24 | G << 16 | B << 8 | 255, from its luma and the chroma it sees (any byte values:
// what leaves 0 .. 255 is clamped).  The largest intermediate is below 2^26.
MM_YUV_FN uint32_t mm_yuv_to_rgba(const mm_yuv_rgba_mode &m, int luma, int cb, int cr) {
    const int y = m.ky * (luma - m.off) + (1 << 15), u = cb - 128, v = cr - 128;
    const int r = mm_yuv_clamp255((y + m.rcr * v) >> 16);
    const int g = mm_yuv_clamp255((y + m.gcb * u + m.gcr * v) >> 16);
    const int b = mm_yuv_clamp255((y + m.bcb * u) >> 16);
    return (uint32_t)r << 24 | (uint32_t)g << 16 | (uint32_t)b << 8 | 255u;
}

// The chroma a pixel sees in bilinear mode, in two exact steps: the column sum of the pixel's own chroma row (3) and its
// neighbour row (1), then the pixel's own column (3) and its neighbour column (1), rounded once:
// (9 C[cy][cx] + 3 C[cy][nx] + 3 C[ny][cx] + C[ny][nx] + 8) >> 4.
MM_YUV_FN int mm_yuv_chroma_column(int own_row, int neighbour_row) { return 3 * own_row + neighbour_row; }
MM_YUV_FN int mm_yuv_chroma_blend(int own_column, int neighbour_column) { return (3 * own_column + neighbour_column + 8) >> 4; }

// Chroma sample index of the neighbour of pixel coordinate p along an axis with n chroma samples: towards the odd
// pixel's right (lower) sample, the even pixel's left (upper) one, clamped to the plane.
MM_YUV_FN int mm_yuv_chroma_neighbour(int p, int n) {
    const int c = (p >> 1) + ((p & 1) ? 1 : -1);
    return c < 0 ? 0 : c > n - 1 ? n - 1 : c;
}

// The chroma pixel (x, y) sees in a plane of cw x ch samples with rows cw apart.
MM_YUV_FN int mm_yuv_chroma_replicate(const unsigned char *plane, int cw, int ch, int x, int y) {
    (void)ch;
    return plane[(int64_t)(y >> 1) * cw + (x >> 1)];
}
MM_YUV_FN int mm_yuv_chroma_bilinear(const unsigned char *plane, int cw, int ch, int x, int y) {
    const int cx = x >> 1, cy = y >> 1, nx = mm_yuv_chroma_neighbour(x, cw), ny = mm_yuv_chroma_neighbour(y, ch);
    const unsigned char *own = plane + (int64_t)cy * cw, *nb = plane + (int64_t)ny * cw;
    return mm_yuv_chroma_blend(mm_yuv_chroma_column(own[cx], nb[cx]), mm_yuv_chroma_column(own[nx], nb[nx]));
}

// A whole frame on the host, as the kernel converts it: src is one frame's payload (mm_yuv_frame_bytes), dst width *
// height words.
inline void mm_yuv_to_rgba_frame_host(const mm_yuv_rgba_mode &m, int chroma, const unsigned char *src, int width, int height, uint32_t *dst) {
    const int cw = mm_yuv_cw(width), ch = mm_yuv_ch(height);
    const unsigned char *cb = src + mm_yuv_cb_offset(width, height), *cr = src + mm_yuv_cr_offset(width, height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const bool rep = chroma == MM_YUV_CHROMA_REPLICATE;
            const int u = rep ? mm_yuv_chroma_replicate(cb, cw, ch, x, y) : mm_yuv_chroma_bilinear(cb, cw, ch, x, y);
            const int v = rep ? mm_yuv_chroma_replicate(cr, cw, ch, x, y) : mm_yuv_chroma_bilinear(cr, cw, ch, x, y);
            dst[(int64_t)y * width + x] = mm_yuv_to_rgba(m, src[(int64_t)y * width + x], u, v);
        }
}

// ---- 10-bit output from float frames: float4 RGBA pixels to planar Y'CbCr 4:2:0 with 16-bit little-endian samples, the
// value in the low 10 bits (k_float_to_yuv420p10_clip, clip_yuv10.hip; the semantics are stated at
// mmhip_clip_float_to_yuv420p10 in include/mmhip.h) ----

// One mode over channels quantised to 0 .. 65535: Y = ((yr R + yg G + yb B + 2^19) >> 20) + off; a chroma sample is
// clamp(((k . sums of the 2 x 2 block) + 2^20) >> 21) + 512.  A luma coefficient is floor(k * E / 65535 * 2^20 + 0.5) with
// the excursion E = 876 (limited) or 1023 (full), a chroma coefficient sign(k) floor(|k| * E / 65535 * 2^19 + 0.5) with
// E = 896 or 1023; the green coefficient of every row makes the row sum exactly (luma: the coefficient of k = 1, chroma:
// 0), so white is 940 or 1023 and grey has chroma 512.  Chroma is at scale 2^19 because at 2^20 the full-range sums of four
// pixels would end 32 736 below 2^31.
static const mm_yuv_mode MM_YUV10_MODES[MM_YUV_MATRICES][MM_YUV_RANGES] = {
    {{64, 4191, 8227, 1598, -1210, -2374, 3584, 3584, -3001, -583},      // bt601 limited
     {0, 4894, 9608, 1866, -1381, -2711, 4092, 4092, -3427, -665}},      // bt601 full
    {{64, 2980, 10024, 1012, -821, -2763, 3584, 3584, -3255, -329},      // bt709 limited
     {0, 3480, 11706, 1182, -938, -3154, 4092, 4092, -3717, -375}},      // bt709 full
};

// One channel: CLAMP01 as the pixel store sees it (NaN and -0 give 0), one float32 product, rounded to nearest with ties
// to even: 0 .. 65535.  The device spells the two operations with intrinsics the compiler neither contracts nor
// reassociates; the host's product is a single float32 multiplication and rintf rounds in the default mode.
MM_YUV_FN int mm_yuv10_quant(float v) {
    const float c = !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v);
#if defined(__HIP_DEVICE_COMPILE__)
    return __float2int_rn(__fmul_rn(c, 65535.0f));
#else
    volatile float p = c * 65535.0f;
    return (int)__builtin_rintf(p);
#endif
}

// The luma of one pixel: 64 .. 940 or 0 .. 1023 by construction, no clamp.  The largest intermediate is 1 073 201 168.
MM_YUV_FN int mm_yuv10_luma(const mm_yuv_mode &m, int r, int g, int b) { return ((m.yr * r + m.yg * g + m.yb * b + (1 << 19)) >> 20) + m.off; }

// One chroma sample from the sums of its block's four pixels.  The intermediates lie in [-1 072 676 880, 1 073 725 456],
// so the sample lies in 1 .. 1023 before the clamp (pure blue and pure red at full range, 1023.5 in the real formula, give
// 1023): the clamp is a guard no colour reaches.
MM_YUV_FN int mm_yuv10_chroma(int kr, int kg, int kb, int rs, int gs, int bs) {
    const int c = ((kr * rs + kg * gs + kb * bs + (1 << 20)) >> 21) + 512;
    return c < 0 ? 0 : c > 1023 ? 1023 : c;
}
MM_YUV_FN int mm_yuv10_cb(const mm_yuv_mode &m, int rs, int gs, int bs) { return mm_yuv10_chroma(m.cbr, m.cbg, m.cbb, rs, gs, bs); }
MM_YUV_FN int mm_yuv10_cr(const mm_yuv_mode &m, int rs, int gs, int bs) { return mm_yuv10_chroma(m.crr, m.crg, m.crb, rs, gs, bs); }

// A frame: the planes of mm_yuv_frame_bytes with two bytes per sample; the plane offsets of mm_yuv_cb_offset and
// mm_yuv_cr_offset count samples.
MM_YUV_FN int64_t mm_yuv10_frame_bytes(int width, int height) { return 2 * mm_yuv_frame_bytes(width, height); }

// A whole frame on the host, as the kernel converts it: src is height rows of width float4 RGBA pixels row_stride bytes
// apart (alpha is not read), dst one frame of mm_yuv10_frame_bytes / 2 samples.  An odd last column or row is
// replicated.
inline void mm_yuv10_frame_host(const mm_yuv_mode &m, const float *src, int64_t row_stride, int width, int height, uint16_t *dst) {
    const int cw = mm_yuv_cw(width), ch = mm_yuv_ch(height);
    uint16_t *cb = dst + mm_yuv_cb_offset(width, height), *cr = dst + mm_yuv_cr_offset(width, height);
    auto pixel = [&](int r, int c) { return (const float *)((const char *)src + r * row_stride) + (int64_t)c * 4; };
    for (int r = 0; r < height; ++r)
        for (int c = 0; c < width; ++c) {
            const float *p = pixel(r, c);
            dst[(int64_t)r * width + c] = (uint16_t)mm_yuv10_luma(m, mm_yuv10_quant(p[0]), mm_yuv10_quant(p[1]), mm_yuv10_quant(p[2]));
        }
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            int rs = 0, gs = 0, bs = 0;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const int c = 2 * cx + i < width ? 2 * cx + i : width - 1, r = 2 * cy + j < height ? 2 * cy + j : height - 1;
                    const float *p = pixel(r, c);
                    rs += mm_yuv10_quant(p[0]);
                    gs += mm_yuv10_quant(p[1]);
                    bs += mm_yuv10_quant(p[2]);
                }
            cb[(int64_t)cy * cw + cx] = (uint16_t)mm_yuv10_cb(m, rs, gs, bs);
            cr[(int64_t)cy * cw + cx] = (uint16_t)mm_yuv10_cr(m, rs, gs, bs);
        }
}

// ---- 10-bit input to float frames: planar Y'CbCr 4:2:0 payloads of 16-bit samples to float4 RGBA texels, what a deep
// drawable binds (k_yuv420p10_to_float_clip, clip_yuv10_in.hip; the semantics are stated at mmhip_clip_from_yuv420p10 in
// include/mmhip.h) ----

// One mode: with yf = (float)(Y - off), uf = (float)(S_cb - 8192), vf = (float)(S_cr - 8192) -- S the chroma the pixel sees
// at scale 16 -- and L = yf / e,
//   R = L + vf * rcr, G = (L + uf * gcb) + vf * gcr, B = L + uf * bcb,
// every operation one float32 operation rounded to nearest.  Each coefficient is the float32 nearest to the exact
// rational 2 (1 - Kr) / (16 Ec) and so on, Ec = 896 (limited) or 1023 (full).
struct mm_yuv10_float_mode {
    int off;
    float e, rcr, gcb, gcr, bcb;
};

// [matrix][range]
static const mm_yuv10_float_mode MM_YUV10_FLOAT_MODES[MM_YUV_MATRICES][MM_YUV_RANGES] = {
    {{64, 876.0f, 0x1.9a2f66p-14f, -0x1.92bce0p-16f, -0x1.a1df2ap-15f, 0x1.0337e2p-13f},      // bt601 limited
     {0, 1023.0f, 0x1.67434ap-14f, -0x1.60bd72p-16f, -0x1.6dfec6p-15f, 0x1.c61350p-14f}},     // bt601 full
    {{64, 876.0f, 0x1.ccbdd2p-14f, -0x1.b67222p-17f, -0x1.11eb6ap-15f, 0x1.0f72a2p-13f},      // bt709 limited
     {0, 1023.0f, 0x1.938afap-14f, -0x1.8003e0p-17f, -0x1.dfd3eep-16f, 0x1.db7f7ap-14f}},     // bt709 full
};

// The three float32 operations.  The device spells them with intrinsics the compiler neither contracts nor
// reassociates; the host forms each result in a volatile, so that no product meets a sum in an fma.
#if defined(__HIP_DEVICE_COMPILE__)
MM_YUV_FN float mm_yuv_fmul(float a, float b) { return __fmul_rn(a, b); }
MM_YUV_FN float mm_yuv_fadd(float a, float b) { return __fadd_rn(a, b); }
MM_YUV_FN float mm_yuv_fdiv(float a, float b) { return __fdiv_rn(a, b); }
#else
MM_YUV_FN float mm_yuv_fmul(float a, float b) { volatile float r = a * b; return r; }
MM_YUV_FN float mm_yuv_fadd(float a, float b) { volatile float r = a + b; return r; }
MM_YUV_FN float mm_yuv_fdiv(float a, float b) { volatile float r = a / b; return r; }
#endif

// A sample as it is read: nothing is refused, what lies above 10 bits is 1023.
MM_YUV_FN int mm_yuv10_sample(unsigned s) { return (int)(s < 1023u ? s : 1023u); }

// The chroma a pixel sees at scale 16, an exact integer in 0 .. 16 368: mm_yuv_chroma_column's sums of the own and the
// neighbour column weighed 3 and 1 without the rounding of mm_yuv_chroma_blend; replicate mode is 16 times the sample.
MM_YUV_FN int mm_yuv10_chroma_blend16(int own_column, int neighbour_column) { return 3 * own_column + neighbour_column; }
MM_YUV_FN int mm_yuv10_chroma_replicate16(int sample) { return 16 * sample; }

// One pixel's texel from its luma (0 .. 1023) and the chroma it sees at scale 16.  Nothing is clamped.
MM_YUV_FN void mm_yuv10_to_float(const mm_yuv10_float_mode &m, int luma, int s_cb, int s_cr, float rgba[4]) {
    const float yf = (float)(luma - m.off), uf = (float)(s_cb - 8192), vf = (float)(s_cr - 8192);
    const float l = mm_yuv_fdiv(yf, m.e);
    rgba[0] = mm_yuv_fadd(l, mm_yuv_fmul(vf, m.rcr));
    rgba[1] = mm_yuv_fadd(mm_yuv_fadd(l, mm_yuv_fmul(uf, m.gcb)), mm_yuv_fmul(vf, m.gcr));
    rgba[2] = mm_yuv_fadd(l, mm_yuv_fmul(uf, m.bcb));
    rgba[3] = 1.0f;
}

// The chroma at scale 16 pixel (x, y) sees in a plane of cw x ch samples with rows cw apart.
MM_YUV_FN int mm_yuv10_chroma16(int chroma, const uint16_t *plane, int cw, int ch, int x, int y) {
    const int cx = x >> 1, cy = y >> 1;
    const uint16_t *own = plane + (int64_t)cy * cw;
    if (chroma == MM_YUV_CHROMA_REPLICATE) return mm_yuv10_chroma_replicate16(mm_yuv10_sample(own[cx]));
    const int nx = mm_yuv_chroma_neighbour(x, cw), ny = mm_yuv_chroma_neighbour(y, ch);
    const uint16_t *nb = plane + (int64_t)ny * cw;
    return mm_yuv10_chroma_blend16(mm_yuv_chroma_column(mm_yuv10_sample(own[cx]), mm_yuv10_sample(nb[cx])),
                                   mm_yuv_chroma_column(mm_yuv10_sample(own[nx]), mm_yuv10_sample(nb[nx])));
}

// A whole frame on the host, as the kernel converts it: src is one frame's payload (mm_yuv10_frame_bytes / 2 samples in
// the host's byte order), dst width * height float4 texels.
inline void mm_yuv10_to_float_frame_host(const mm_yuv10_float_mode &m, int chroma, const uint16_t *src, int width, int height, float *dst) {
    const int cw = mm_yuv_cw(width), ch = mm_yuv_ch(height);
    const uint16_t *cb = src + mm_yuv_cb_offset(width, height), *cr = src + mm_yuv_cr_offset(width, height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x)
            mm_yuv10_to_float(m, mm_yuv10_sample(src[(int64_t)y * width + x]), mm_yuv10_chroma16(chroma, cb, cw, ch, x, y),
                              mm_yuv10_chroma16(chroma, cr, cw, ch, x, y), dst + ((int64_t)y * width + x) * 4);
}

// ---- left-sited chroma (MPEG-2 siting, C420mpeg2: what H.264, HEVC and AV1 streams carry under BT.709 and BT.601): a
// chroma sample is co-sited with the even luma column of its block and lies between the block's two rows.  The
// semantics are stated at mmhip_clip_to_yuv420_sited and its three siblings in include/mmhip.h; everything above is the
// centre siting (C420jpeg) and stays what it is.  Luma, the coefficient tables, the layout and everything after the chroma
// a pixel sees are shared with the centre functions. ----
enum { MM_YUV_SITING_CENTER = 0, MM_YUV_SITING_LEFT = 1, MM_YUV_SITINGS = 2 };

inline bool mm_yuv_siting_known(int siting) { return siting >= 0 && siting < MM_YUV_SITINGS; }

// Out: the weighted sum of a channel over the six pixels of chroma sample (cx, cy), from the sums over the two rows of
// the pixel columns 2 cx - 1, 2 cx and 2 cx + 1 (clamped to the frame): weights 1, 2, 1 per row, 8 in all.
MM_YUV_FN int mm_yuv_left_sum(int left_column, int own_column, int right_column) { return left_column + 2 * own_column + right_column; }

// One 8-bit chroma sample from the weighted sums (at most 8 * 255 = 2040 each).  The absolute coefficients of a row sum to
// at most 65 536 (bt601 and bt709 full: 32768 + 27439 + 5329, 32768 + 29763 + 3005), so |k . sums| <= 65 536 * 2040 =
// 133 693 440 and with the rounding term 2^18 the intermediate stays below 2^27: an int holds it.  A row sums to 0, so grey
// gives (2^18 >> 19) + 128 = 128.
MM_YUV_FN int mm_yuv_chroma_left(int kr, int kg, int kb, int rs, int gs, int bs) {
    const int c = ((kr * rs + kg * gs + kb * bs + (1 << 18)) >> 19) + 128;
    return c < 0 ? 0 : c > 255 ? 255 : c;
}
MM_YUV_FN int mm_yuv_cb_left(const mm_yuv_mode &m, int rs, int gs, int bs) { return mm_yuv_chroma_left(m.cbr, m.cbg, m.cbb, rs, gs, bs); }
MM_YUV_FN int mm_yuv_cr_left(const mm_yuv_mode &m, int rs, int gs, int bs) { return mm_yuv_chroma_left(m.crr, m.crg, m.crb, rs, gs, bs); }

// One 10-bit chroma sample from the weighted sums of mm_yuv10_quant values (at most 8 * 65535 = 524 280 each).  A row
// has coefficients of both signs that sum to 0, so k . sums is largest where the channels of the positive coefficients
// are full and the others 0: within +-4092 * 524 280 = +-2 145 353 760, and every partial sum within that too.  With the
// rounding term 2^21 the intermediate lies in [-2 143 256 608, 2 147 450 912]: twice the centre form's, and its upper end
// 32 736 below 2^31 -- the very margin the centre form goes to scale 2^19 to avoid.  An int32 would hold it, by that
// hair and for these tables only; the products are formed and summed in int64, where nothing hangs on the margin.  The
// shift is a floor division; it leaves -511 .. 511, so the sample lies in 1 .. 1023 before the clamp.  Grey gives 512.
MM_YUV_FN int mm_yuv10_chroma_left(int kr, int kg, int kb, int rs, int gs, int bs) {
    const int64_t t = (int64_t)kr * rs + (int64_t)kg * gs + (int64_t)kb * bs + ((int64_t)1 << 21);
    const int c = (int)(t >> 22) + 512;
    return c < 0 ? 0 : c > 1023 ? 1023 : c;
}
MM_YUV_FN int mm_yuv10_cb_left(const mm_yuv_mode &m, int rs, int gs, int bs) { return mm_yuv10_chroma_left(m.cbr, m.cbg, m.cbb, rs, gs, bs); }
MM_YUV_FN int mm_yuv10_cr_left(const mm_yuv_mode &m, int rs, int gs, int bs) { return mm_yuv10_chroma_left(m.crr, m.crg, m.crb, rs, gs, bs); }

// In, bilinear: an even pixel column lies on its chroma column, an odd one half way to the next.  Chroma column of the
// right neighbour of pixel column x, clamped to the plane; and the horizontal step over mm_yuv_chroma_column's sums,
// weights 4 | 2, 2 of 16 in all: rounded once at 8 bits, kept at scale 16 at 10.
MM_YUV_FN int mm_yuv_chroma_right(int x, int cw) {
    const int r = (x >> 1) + 1;
    return r > cw - 1 ? cw - 1 : r;
}
MM_YUV_FN int mm_yuv10_chroma_blend16_left(int own_column, int right_column, int odd) { return odd ? 2 * own_column + 2 * right_column : 4 * own_column; }
MM_YUV_FN int mm_yuv_chroma_blend_left(int own_column, int right_column, int odd) {
    return (mm_yuv10_chroma_blend16_left(own_column, right_column, odd) + 8) >> 4;
}

// The chroma pixel (x, y) sees in a plane of cw x ch samples with rows cw apart, left siting.
MM_YUV_FN int mm_yuv_chroma_bilinear_left(const unsigned char *plane, int cw, int ch, int x, int y) {
    const int cx = x >> 1, cy = y >> 1, rx = mm_yuv_chroma_right(x, cw), ny = mm_yuv_chroma_neighbour(y, ch);
    const unsigned char *own = plane + (int64_t)cy * cw, *nb = plane + (int64_t)ny * cw;
    return mm_yuv_chroma_blend_left(mm_yuv_chroma_column(own[cx], nb[cx]), mm_yuv_chroma_column(own[rx], nb[rx]), x & 1);
}
MM_YUV_FN int mm_yuv10_chroma16_left(const uint16_t *plane, int cw, int ch, int x, int y) {
    const int cx = x >> 1, cy = y >> 1, rx = mm_yuv_chroma_right(x, cw), ny = mm_yuv_chroma_neighbour(y, ch);
    const uint16_t *own = plane + (int64_t)cy * cw, *nb = plane + (int64_t)ny * cw;
    return mm_yuv10_chroma_blend16_left(mm_yuv_chroma_column(mm_yuv10_sample(own[cx]), mm_yuv10_sample(nb[cx])),
                                        mm_yuv_chroma_column(mm_yuv10_sample(own[rx]), mm_yuv10_sample(nb[rx])), x & 1);
}

// Whole frames on the host with a siting, as the kernels convert them: MM_YUV_SITING_CENTER is the functions above.  The
// arguments are theirs.
inline void mm_yuv_frame_host_sited(const mm_yuv_mode &m, int siting, const unsigned char *rgba, int64_t row_stride, int width, int height,
                                    unsigned char *dst) {
    mm_yuv_frame_host(m, rgba, row_stride, width, height, dst);
    if (siting != MM_YUV_SITING_LEFT) return;
    const int cw = mm_yuv_cw(width), ch = mm_yuv_ch(height);
    unsigned char *cb = dst + mm_yuv_cb_offset(width, height), *cr = dst + mm_yuv_cr_offset(width, height);
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            int s[3][3];      // [column][channel]
            for (int i = 0; i < 3; ++i) {
                const int x = 2 * cx - 1 + i, c = x < 0 ? 0 : x < width ? x : width - 1;
                s[i][0] = s[i][1] = s[i][2] = 0;
                for (int j = 0; j < 2; ++j) {
                    const int r = 2 * cy + j < height ? 2 * cy + j : height - 1;
                    const unsigned char *p = rgba + r * row_stride + (int64_t)c * 4;
                    for (int k = 0; k < 3; ++k) s[i][k] += p[k];
                }
            }
            const int rs = mm_yuv_left_sum(s[0][0], s[1][0], s[2][0]), gs = mm_yuv_left_sum(s[0][1], s[1][1], s[2][1]),
                      bs = mm_yuv_left_sum(s[0][2], s[1][2], s[2][2]);
            cb[(int64_t)cy * cw + cx] = (unsigned char)mm_yuv_cb_left(m, rs, gs, bs);
            cr[(int64_t)cy * cw + cx] = (unsigned char)mm_yuv_cr_left(m, rs, gs, bs);
        }
}

inline void mm_yuv10_frame_host_sited(const mm_yuv_mode &m, int siting, const float *src, int64_t row_stride, int width, int height, uint16_t *dst) {
    mm_yuv10_frame_host(m, src, row_stride, width, height, dst);
    if (siting != MM_YUV_SITING_LEFT) return;
    const int cw = mm_yuv_cw(width), ch = mm_yuv_ch(height);
    uint16_t *cb = dst + mm_yuv_cb_offset(width, height), *cr = dst + mm_yuv_cr_offset(width, height);
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            int s[3][3];      // [column][channel]
            for (int i = 0; i < 3; ++i) {
                const int x = 2 * cx - 1 + i, c = x < 0 ? 0 : x < width ? x : width - 1;
                s[i][0] = s[i][1] = s[i][2] = 0;
                for (int j = 0; j < 2; ++j) {
                    const int r = 2 * cy + j < height ? 2 * cy + j : height - 1;
                    const float *p = (const float *)((const char *)src + r * row_stride) + (int64_t)c * 4;
                    for (int k = 0; k < 3; ++k) s[i][k] += mm_yuv10_quant(p[k]);
                }
            }
            const int rs = mm_yuv_left_sum(s[0][0], s[1][0], s[2][0]), gs = mm_yuv_left_sum(s[0][1], s[1][1], s[2][1]),
                      bs = mm_yuv_left_sum(s[0][2], s[1][2], s[2][2]);
            cb[(int64_t)cy * cw + cx] = (uint16_t)mm_yuv10_cb_left(m, rs, gs, bs);
            cr[(int64_t)cy * cw + cx] = (uint16_t)mm_yuv10_cr_left(m, rs, gs, bs);
        }
}

inline void mm_yuv_to_rgba_frame_host_sited(const mm_yuv_rgba_mode &m, int chroma, int siting, const unsigned char *src, int width, int height,
                                            uint32_t *dst) {
    if (siting != MM_YUV_SITING_LEFT || chroma == MM_YUV_CHROMA_REPLICATE) return mm_yuv_to_rgba_frame_host(m, chroma, src, width, height, dst);
    const int cw = mm_yuv_cw(width), ch = mm_yuv_ch(height);
    const unsigned char *cb = src + mm_yuv_cb_offset(width, height), *cr = src + mm_yuv_cr_offset(width, height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x)
            dst[(int64_t)y * width + x] = mm_yuv_to_rgba(m, src[(int64_t)y * width + x], mm_yuv_chroma_bilinear_left(cb, cw, ch, x, y),
                                                         mm_yuv_chroma_bilinear_left(cr, cw, ch, x, y));
}

inline void mm_yuv10_to_float_frame_host_sited(const mm_yuv10_float_mode &m, int chroma, int siting, const uint16_t *src, int width, int height,
                                               float *dst) {
    if (siting != MM_YUV_SITING_LEFT || chroma == MM_YUV_CHROMA_REPLICATE) return mm_yuv10_to_float_frame_host(m, chroma, src, width, height, dst);
    const int cw = mm_yuv_cw(width), ch = mm_yuv_ch(height);
    const uint16_t *cb = src + mm_yuv_cb_offset(width, height), *cr = src + mm_yuv_cr_offset(width, height);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x)
            mm_yuv10_to_float(m, mm_yuv10_sample(src[(int64_t)y * width + x]), mm_yuv10_chroma16_left(cb, cw, ch, x, y),
                              mm_yuv10_chroma16_left(cr, cw, ch, x, y), dst + ((int64_t)y * width + x) * 4);
}
