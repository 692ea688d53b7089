// The arithmetic of a clip's reconstruction filter (k_filter_combine_clip, clip_combine.hip; the semantics are stated
// at mmhip_render_clip_filtered in include/mmhip.h): the kernel functions of one axis in double, the normalised float
// taps of a pixel's edge class, and the two sequential f32 sums -- along the row into h_b, down the column into s_j.
// Plain C++, so that the host compiles the same text: the runtime builds the tap tables with it, the combine kernel sums
// with its steps, and a stand-alone test program (tests/test_clip_filtered_api.py) runs the whole of it on a frame
// worked out by hand.  Compile without floating-point contraction: no product may join its sum in an fma.
#pragma once
#include <math.h>

#if defined(__HIP__)
#define MM_CLIP_FILTER_FN __attribute__((host)) __attribute__((device)) inline
#else
#define MM_CLIP_FILTER_FN inline
#endif

enum { MM_CLIP_FILTER_BOX = 0, MM_CLIP_FILTER_TENT = 1, MM_CLIP_FILTER_GAUSSIAN = 2, MM_CLIP_FILTER_MITCHELL = 3, MM_CLIP_FILTER_KERNELS = 4 };
enum { MM_CLIP_FILTER_MAX_REACH = 4 };      // neighbour pixels on each side at the largest radius

// D: the neighbour pixels a filter of `radius` pixels reaches on each side (radius is 0.5 .. 4, so D is 0 .. 4).
inline int mm_clip_filter_reach(double radius) { return (int)ceil(radius - 0.5); }

// The weight of one axis at distance d from the pixel centre, before normalisation.  Every expression in the order it
// is evaluated; the cubics in Horner form.
inline double mm_clip_filter_k(int kernel, double d, double radius) {
    const double ad = fabs(d);
    if (ad >= radius) return 0.0;
    if (kernel == MM_CLIP_FILTER_BOX) return 1.0;
    if (kernel == MM_CLIP_FILTER_TENT) return 1.0 - ad / radius;
    if (kernel == MM_CLIP_FILTER_GAUSSIAN) return exp(-2.0 * (d * d)) - exp(-2.0 * (radius * radius));
    // Mitchell-Netravali, B = C = 1/3, the support [-2, 2] stretched to the radius
    const double u = (2.0 * ad) / radius;
    if (u < 1.0) return (((7.0 * u - 12.0) * u) * u + 16.0 / 3.0) / 6.0;
    return ((((-7.0 / 3.0) * u + 12.0) * u - 20.0) * u + 32.0 / 3.0) / 6.0;
}

// The taps of one axis: tap (dx, a), dx = -D .. D and a = 0 .. n - 1, has the index (dx + D) * n + a.
MM_CLIP_FILTER_FN int mm_clip_filter_tap_count(int reach, int n) { return (2 * reach + 1) * n; }

// The edge class of the pixel at index `at` of an axis of `size` pixels: lo neighbours before it and hi after it inside
// the frame, each at most D.  Class lo * (D + 1) + hi; the interior is D * (D + 1) + D.
MM_CLIP_FILTER_FN int mm_clip_filter_class(int at, int size, int reach) {
    const int lo = at < reach ? at : reach, after = size - 1 - at, hi = after < reach ? after : reach;
    return lo * (reach + 1) + hi;
}

// The normalised float taps of a pixel with lo neighbours before it and hi after it: out[mm_clip_filter_tap_count(D, n)].
// `offsets`: the n sampling offsets of the axis (mm_sample_grid_offset).  The norm is the double sum of k over the
// existing taps in tap order, a tap is (float)(k / norm), and a tap that does not exist is 0, like one that rounds to
// 0: such taps are never read.  Returns 0, or -1 where the norm is not a positive finite number.
inline int mm_clip_filter_taps(int kernel, double radius, int n, const float *offsets, int lo, int hi, float *out) {
    const int reach = mm_clip_filter_reach(radius);
    double norm = 0.0;
    for (int dx = -lo; dx <= hi; ++dx)
        for (int a = 0; a < n; ++a) norm = norm + mm_clip_filter_k(kernel, (double)dx + (double)offsets[a], radius);
    if (!(norm > 0.0) || !(norm <= 1.7976931348623157e308)) return -1;
    for (int dx = -reach; dx <= reach; ++dx)
        for (int a = 0; a < n; ++a) {
            const bool exists = dx >= -lo && dx <= hi;
            out[(dx + reach) * n + a] = exists ? (float)(mm_clip_filter_k(kernel, (double)dx + (double)offsets[a], radius) / norm) : 0.0f;
        }
    return 0;
}

// What the combine kernel reads of a table: only the taps that are read, in tap order.  words[0] is their count, words[1
// + t] the weight of the t-th of them (the float's bits) and words[1 + taps + t] its place, (dx + D) << 8 | a, with taps =
// mm_clip_filter_tap_count(D, n); a block has mm_clip_filter_block_words(taps) words.
MM_CLIP_FILTER_FN int mm_clip_filter_block_words(int taps) { return 1 + 2 * taps; }
inline void mm_clip_filter_compact(const float *dense, int reach, int n, unsigned *words) {
    const int taps = mm_clip_filter_tap_count(reach, n);
    unsigned count = 0;
    for (int t = 0; t < taps; ++t)
        if (dense[t] != 0.0f) {
            words[1 + count] = __builtin_bit_cast(unsigned, dense[t]);
            words[1 + taps + count] = (unsigned)(t / n) << 8 | (unsigned)(t % n);
            ++count;
        }
    words[0] = count;
    for (unsigned t = count; t < (unsigned)taps; ++t) words[1 + t] = words[1 + taps + t] = 0u;
}

// The blocks of every edge class of an axis of `size` pixels, (D + 1)^2 of them behind `words`.  Only the first and the last
// D pixels of an axis differ from the interior; a class no pixel of the axis has is an empty block, whatever its weights
// would sum to.  Returns 0, or -1 where the weights of a class that occurs do not sum to a positive finite number.
inline int mm_clip_filter_axis_blocks(int kernel, double radius, int n, const float *offsets, int size, unsigned *words) {
    const int reach = mm_clip_filter_reach(radius), taps = mm_clip_filter_tap_count(reach, n), block = mm_clip_filter_block_words(taps);
    const int classes = (reach + 1) * (reach + 1);
    float dense[(2 * MM_CLIP_FILTER_MAX_REACH + 1) * 8];
    for (int i = 0; i < classes * block; ++i) words[i] = 0u;
    for (int pass = 0; pass < 2; ++pass) {
        const int from = pass == 0 ? 0 : (size - 1 - reach > 0 ? size - 1 - reach : 0);
        const int to = pass == 0 ? (size - 1 < reach ? size - 1 : reach) : size - 1;
        for (int at = from; at <= to; ++at) {
            const int cls = mm_clip_filter_class(at, size, reach);
            if (mm_clip_filter_taps(kernel, radius, n, offsets, cls / (reach + 1), cls % (reach + 1), dense) != 0) return -1;
            mm_clip_filter_compact(dense, reach, n, words + cls * block);
        }
    }
    return 0;
}

// One channel of either sum: the first product starts it, every later one is added to it; each product is rounded on
// its own.
MM_CLIP_FILTER_FN float mm_clip_filter_first(float w, float f) { return w * f; }
MM_CLIP_FILTER_FN float mm_clip_filter_next(float acc, float w, float f) {
    const float p = w * f;
    return acc + p;
}

// One time step of one frame on the host, the two sums as the kernel makes them: maps[b * sx + a] is the sub-sample map
// of grid point (b, a), float [height][width][4] over the whole frame; tx and ty are the tap tables of every edge class
// ((D + 1)^2 tables of mm_clip_filter_tap_count floats each); h is scratch of sy * height * width * 4 floats; s, float
// [height][width][4], receives s_j.  A tap of weight 0 is not read.
inline void mm_clip_filter_step_host(const float *const *maps, int width, int height, int sx, int sy, int reach, const float *tx,
                                     const float *ty, float *h, float *s) {
    const int taps_x = mm_clip_filter_tap_count(reach, sx), taps_y = mm_clip_filter_tap_count(reach, sy);
    for (int b = 0; b < sy; ++b)
        for (int r = 0; r < height; ++r)
            for (int c = 0; c < width; ++c) {
                const float *w = tx + mm_clip_filter_class(c, width, reach) * taps_x;
                for (int ch = 0; ch < 4; ++ch) {
                    float acc = 0.0f;
                    bool any = false;
                    for (int dx = -reach; dx <= reach; ++dx)
                        for (int a = 0; a < sx; ++a) {
                            const float wt = w[(dx + reach) * sx + a];
                            if (wt == 0.0f) continue;
                            const float f = maps[b * sx + a][((long)r * width + (c + dx)) * 4 + ch];
                            acc = any ? mm_clip_filter_next(acc, wt, f) : mm_clip_filter_first(wt, f);
                            any = true;
                        }
                    h[(((long)b * height + r) * width + c) * 4 + ch] = acc;
                }
            }
    for (int r = 0; r < height; ++r)
        for (int c = 0; c < width; ++c) {
            const float *w = ty + mm_clip_filter_class(r, height, reach) * taps_y;
            for (int ch = 0; ch < 4; ++ch) {
                float acc = 0.0f;
                bool any = false;
                for (int dy = -reach; dy <= reach; ++dy)
                    for (int b = 0; b < sy; ++b) {
                        const float wt = w[(dy + reach) * sy + b];
                        if (wt == 0.0f) continue;
                        const float f = h[(((long)b * height + (r + dy)) * width + c) * 4 + ch];
                        acc = any ? mm_clip_filter_next(acc, wt, f) : mm_clip_filter_first(wt, f);
                        any = true;
                    }
                s[((long)r * width + c) * 4 + ch] = acc;
            }
        }
}
