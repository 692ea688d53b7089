// Planar Y'CbCr 4:2:0 frames of 16-bit samples to the float4 texels of a deep input drawable (mmhip_clip_from_yuv420p10 in
// include/mmhip.h states the semantics, mm_yuv.h holds the arithmetic and the layout): the mirror image of
// clip_yuv10.hip and the float sibling of clip_yuv_in.hip.  One launch over (tiles of a frame, frames), the frames in HBM
// on both sides.
#include <hip/hip_runtime.h>

#include "mm_yuv.h"
#include "clip_yuv_common.h"

namespace mm {

// Frame blockIdx.y of the call per grid row, 256 work-items per workgroup; a work-item owns whole 2 x 2 blocks, so no
// texel of the output is written by two of them.  Offsets inside a frame are 32-bit from the frame's 64-bit bases, which
// are uniform over the workgroup: sample offsets into the planes, texel offsets into the destination; the launcher
// refuses a destination frame of more than 4 GiB (2^28 texels; a source frame is 3/16 of it).
//   COLS = 2, 4, 8 a work-item converts COLS columns of a row pair: per row one Y load of 2 * COLS bytes and COLS 16-byte
//                  stores of 16 * COLS contiguous bytes (a wave writes 2, 4 or 8 KiB contiguous per row); one load of COLS
//                  bytes each of Cb and Cr.  In bilinear mode it reads the chroma rows cy - 1 .. cy + 1 and, next to its
//                  COLS / 2 columns, the columns to their left and right with clamped 2-byte loads (neighbours' cache
//                  lines: nothing is staged through LDS).  The launcher takes it where the width is a multiple of 8 and
//                  the source is aligned for 16-byte accesses (the destination always is).
//   COLS = 0       a work-item converts one 2 x 2 block with clamped 2-byte loads and per-pixel 16-byte stores: any
//                  width, height and 2-byte aligned source.
// All convert with mm_yuv.h's functions and give the same floats.  The last row pair of an odd height has one row and the
// last block of an odd width one column: they are converted once and nothing is stored outside the frame.  The kernel
// writes 16 bytes and reads 3 per pixel: it is bound by its stores, hence the A/B of their flavour (NT).
struct Yuv10InArgs {
    const uint16_t *src;
    float *dst;
    long long src_frame_samples, dst_frame_stride;      // samples; bytes
    unsigned cb_offset, cr_offset;                      // samples
    unsigned width, height, cw, ch;
    unsigned per_pair, items;      // work-items of a row pair and of a frame
    mm_yuv10_float_mode m;
};

// N samples in one load, as 32-bit words of two samples each (the even one low: little-endian; one sample alone in the
// low half)
template <int N>
__device__ __forceinline__ void yuv10_in_load(const uint16_t *p, unsigned w[(N + 1) / 2]) {
    if constexpr (N == 1) w[0] = *p;
    else if constexpr (N == 2) w[0] = *(const unsigned *)p;
    else if constexpr (N == 4) {
        const yuv_u32x2 v = *(const yuv_u32x2 *)p;
        w[0] = v.x;
        w[1] = v.y;
    } else {
        static_assert(N == 8, "a load of 2, 4, 8 or 16 bytes");
        const yuv_u32x4 v = *(const yuv_u32x4 *)p;
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
}
// sample k of such words, as it is read
__device__ __forceinline__ int yuv10_in_sample(const unsigned *w, int k) { return mm_yuv10_sample((w[k >> 1] >> (16 * (k & 1))) & 0xffffu); }

// One texel from a pixel's luma and the chroma it sees at scale 16
template <bool NT>
__device__ __forceinline__ void yuv10_in_store(const mm_yuv10_float_mode &m, int luma, int s_cb, int s_cr, yuv_f32x4 *p) {
    float t[4];
    mm_yuv10_to_float(m, luma, s_cb, s_cr, t);
    const yuv_f32x4 v = {t[0], t[1], t[2], t[3]};
    yuv_store<NT>(v, p);
}

// The column sums of one plane for one pixel row over the work-item's own NC = COLS / 2 chroma columns from `first` and
// their neighbours: the pixel row's own chroma row `own` weighs 3, its neighbour row `nb` 1.  Centre siting takes NC + 2,
// from first - 1 on; left siting NC + 1, from first on (below).  lo and hi are the clamped columns first - 1 and first + NC.
template <int NC, int SITING>
__device__ __forceinline__ void yuv10_in_columns(const uint16_t *__restrict__ P, unsigned own, unsigned nb, unsigned first, unsigned lo, unsigned hi,
                                                 int *col) {
    constexpr int L = SITING == MM_YUV_SITING_LEFT ? 0 : 1;
    unsigned a[(NC + 1) / 2], b[(NC + 1) / 2];
    yuv10_in_load<NC>(P + (own + first), a);
    yuv10_in_load<NC>(P + (nb + first), b);
    if (L) col[0] = mm_yuv_chroma_column(mm_yuv10_sample(P[own + lo]), mm_yuv10_sample(P[nb + lo]));
#pragma unroll
    for (int k = 0; k < NC; ++k) col[L + k] = mm_yuv_chroma_column(yuv10_in_sample(a, k), yuv10_in_sample(b, k));
    col[L + NC] = mm_yuv_chroma_column(mm_yuv10_sample(P[own + hi]), mm_yuv10_sample(P[nb + hi]));
}

// COLS texels of one row from the row's luma words and the chroma each pixel sees
template <int COLS, bool NT>
__device__ __forceinline__ void yuv10_in_row(const mm_yuv10_float_mode &m, const unsigned *y, const int *u, const int *v, yuv_f32x4 *out) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) yuv10_in_store<NT>(m, yuv10_in_sample(y, k), u[k], v[k], out + k);
}

// Left siting (SITING = MM_YUV_SITING_LEFT, bilinear mode only; mmhip_clip_from_yuv420p10_sited): an even pixel column
// lies on its chroma column and an odd one half way to the next, so a work-item needs its own NC chroma columns and the one
// to their right, first + NC clamped to the plane, and nothing to their left: NC + 1 column sums per plane and pixel row
// where centre siting takes NC + 2.  Replicate mode ignores the siting: the launcher takes the centre instantiation.
template <int COLS, int CHROMA, bool NT, int SITING = MM_YUV_SITING_CENTER>
__global__ void __launch_bounds__(256) k_yuv420p10_to_float_clip(const Yuv10InArgs a) {
    constexpr bool LEFT = SITING == MM_YUV_SITING_LEFT;
    const unsigned item = yuv_item();
    if (item >= a.items) return;
    const unsigned cy = item / a.per_pair, at = item - cy * a.per_pair;      // cy < ch: items = per_pair * ch
    const unsigned r0 = 2u * cy;
    const bool two = r0 + 1u < a.height;
    const size_t fi = blockIdx.y;
    const uint16_t *__restrict__ Y = a.src + fi * a.src_frame_samples;
    const uint16_t *__restrict__ CB = Y + a.cb_offset, *__restrict__ CR = Y + a.cr_offset;
    yuv_f32x4 *__restrict__ D = (yuv_f32x4 *)((unsigned char *)a.dst + fi * a.dst_frame_stride);
    const mm_yuv10_float_mode m = a.m;
    // the chroma rows above and below, clamped to the plane: what the upper and the lower pixel row blend with
    const unsigned own = cy * a.cw, up = (cy ? cy - 1u : 0u) * a.cw, down = (cy + 1u < a.ch ? cy + 1u : cy) * a.cw;
    static_assert(!LEFT || CHROMA == MM_YUV_CHROMA_BILINEAR, "replicate mode has no siting");
    if constexpr (COLS != 0) {
        constexpr int NC = COLS / 2;
        const unsigned yo = r0 * a.width + at * COLS, first = at * NC;      // below 2^28: a destination frame is at most 4 GiB
        unsigned y_top[NC], y_bot[NC];
        yuv10_in_load<COLS>(Y + yo, y_top);
        if (two) yuv10_in_load<COLS>(Y + (yo + a.width), y_bot);
        int u[COLS], v[COLS];
        if constexpr (CHROMA == MM_YUV_CHROMA_REPLICATE) {
            unsigned cb[(NC + 1) / 2], cr[(NC + 1) / 2];
            yuv10_in_load<NC>(CB + (own + first), cb);
            yuv10_in_load<NC>(CR + (own + first), cr);
#pragma unroll
            for (int k = 0; k < COLS; ++k) {
                u[k] = mm_yuv10_chroma_replicate16(yuv10_in_sample(cb, k >> 1));
                v[k] = mm_yuv10_chroma_replicate16(yuv10_in_sample(cr, k >> 1));
            }
            yuv10_in_row<COLS, NT>(m, y_top, u, v, D + yo);
            if (two) yuv10_in_row<COLS, NT>(m, y_bot, u, v, D + (yo + a.width));
        } else {
            const unsigned lo = first ? first - 1u : 0u, hi = first + NC < a.cw ? first + NC : a.cw - 1u;
            int cu[NC + (LEFT ? 1 : 2)], cv[NC + (LEFT ? 1 : 2)];
            if constexpr (LEFT) {
                // pixel k has its own column at index k / 2 of the NC + 1, an odd one its right neighbour one further
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j && !two) break;
                    yuv10_in_columns<NC, SITING>(CB, own, j ? down : up, first, lo, hi, cu);
                    yuv10_in_columns<NC, SITING>(CR, own, j ? down : up, first, lo, hi, cv);
#pragma unroll
                    for (int k = 0; k < COLS; ++k) {
                        u[k] = mm_yuv10_chroma_blend16_left(cu[k >> 1], cu[(k >> 1) + 1], k & 1);
                        v[k] = mm_yuv10_chroma_blend16_left(cv[k >> 1], cv[(k >> 1) + 1], k & 1);
                    }
                    yuv10_in_row<COLS, NT>(m, j ? y_bot : y_top, u, v, D + (yo + (j ? a.width : 0u)));
                }
            } else {
                // pixel k has its own column at index 1 + k / 2 of the NC + 2, its neighbour one to the left (k even) or right
                yuv10_in_columns<NC, SITING>(CB, own, up, first, lo, hi, cu);
                yuv10_in_columns<NC, SITING>(CR, own, up, first, lo, hi, cv);
#pragma unroll
                for (int k = 0; k < COLS; ++k) {
                    const int c = 1 + (k >> 1), n = (k & 1) ? c + 1 : c - 1;
                    u[k] = mm_yuv10_chroma_blend16(cu[c], cu[n]);
                    v[k] = mm_yuv10_chroma_blend16(cv[c], cv[n]);
                }
                yuv10_in_row<COLS, NT>(m, y_top, u, v, D + yo);
                if (!two) return;
                yuv10_in_columns<NC, SITING>(CB, own, down, first, lo, hi, cu);
                yuv10_in_columns<NC, SITING>(CR, own, down, first, lo, hi, cv);
#pragma unroll
                for (int k = 0; k < COLS; ++k) {
                    const int c = 1 + (k >> 1), n = (k & 1) ? c + 1 : c - 1;
                    u[k] = mm_yuv10_chroma_blend16(cu[c], cu[n]);
                    v[k] = mm_yuv10_chroma_blend16(cv[c], cv[n]);
                }
                yuv10_in_row<COLS, NT>(m, y_bot, u, v, D + (yo + a.width));
            }
        }
    } else if constexpr (LEFT) {
        // `at` is the chroma column: pixel columns 2 at and, inside the frame, 2 at + 1
        const unsigned c0 = 2u * at;
        const bool wide = c0 + 1u < a.width;
        const unsigned right = at + 1u < a.cw ? at + 1u : at;
        const unsigned yo = r0 * a.width + c0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            const unsigned nb = j ? down : up;
            const int cu = mm_yuv_chroma_column(mm_yuv10_sample(CB[own + at]), mm_yuv10_sample(CB[nb + at]));
            const int cv = mm_yuv_chroma_column(mm_yuv10_sample(CR[own + at]), mm_yuv10_sample(CR[nb + at]));
            const unsigned o = yo + (j ? a.width : 0u);
            yuv10_in_store<NT>(m, mm_yuv10_sample(Y[o]), mm_yuv10_chroma_blend16_left(cu, cu, 0), mm_yuv10_chroma_blend16_left(cv, cv, 0), D + o);
            if (!wide) continue;
            const int ru = mm_yuv_chroma_column(mm_yuv10_sample(CB[own + right]), mm_yuv10_sample(CB[nb + right]));
            const int rv = mm_yuv_chroma_column(mm_yuv10_sample(CR[own + right]), mm_yuv10_sample(CR[nb + right]));
            yuv10_in_store<NT>(m, mm_yuv10_sample(Y[o + 1u]), mm_yuv10_chroma_blend16_left(cu, ru, 1), mm_yuv10_chroma_blend16_left(cv, rv, 1), D + (o + 1u));
        }
    } else {
        // `at` is the chroma column: pixel columns 2 at and, inside the frame, 2 at + 1
        const unsigned c0 = 2u * at;
        const bool wide = c0 + 1u < a.width;
        const unsigned left = at ? at - 1u : 0u, right = at + 1u < a.cw ? at + 1u : at;
        const unsigned yo = r0 * a.width + c0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            const unsigned nb = j ? down : up;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (i && !wide) break;
                int u, v;
                if (CHROMA == MM_YUV_CHROMA_REPLICATE) {
                    u = mm_yuv10_chroma_replicate16(mm_yuv10_sample(CB[own + at]));
                    v = mm_yuv10_chroma_replicate16(mm_yuv10_sample(CR[own + at]));
                } else {
                    const unsigned nc = i ? right : left;
                    u = mm_yuv10_chroma_blend16(mm_yuv_chroma_column(mm_yuv10_sample(CB[own + at]), mm_yuv10_sample(CB[nb + at])),
                                                mm_yuv_chroma_column(mm_yuv10_sample(CB[own + nc]), mm_yuv10_sample(CB[nb + nc])));
                    v = mm_yuv10_chroma_blend16(mm_yuv_chroma_column(mm_yuv10_sample(CR[own + at]), mm_yuv10_sample(CR[nb + at])),
                                                mm_yuv_chroma_column(mm_yuv10_sample(CR[own + nc]), mm_yuv10_sample(CR[nb + nc])));
                }
                const unsigned o = yo + (j ? a.width : 0u) + (unsigned)i;
                yuv10_in_store<NT>(m, mm_yuv10_sample(Y[o]), u, v, D + o);
            }
        }
    }
}

template <int COLS, int CHROMA>
static void yuv10_in_launch(bool nt, dim3 grid, hipStream_t s, const Yuv10InArgs &a) {
    if (nt) k_yuv420p10_to_float_clip<COLS, CHROMA, true><<<grid, 256, 0, s>>>(a);
    else k_yuv420p10_to_float_clip<COLS, CHROMA, false><<<grid, 256, 0, s>>>(a);
}
template <int COLS>
static void yuv10_in_launch(bool rep, bool nt, dim3 grid, hipStream_t s, const Yuv10InArgs &a) {
    if (rep) yuv10_in_launch<COLS, MM_YUV_CHROMA_REPLICATE>(nt, grid, s, a);
    else yuv10_in_launch<COLS, MM_YUV_CHROMA_BILINEAR>(nt, grid, s, a);
}
template <int COLS>
static void yuv10_in_launch_left(bool nt, dim3 grid, hipStream_t s, const Yuv10InArgs &a) {
    if (nt) k_yuv420p10_to_float_clip<COLS, MM_YUV_CHROMA_BILINEAR, true, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
    else k_yuv420p10_to_float_clip<COLS, MM_YUV_CHROMA_BILINEAR, false, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
}

int check_yuv420p10_to_float_clip(const YuvInJob &j, std::string *err) {
    const YuvRefusal no(j.name, err);
    if (yuv_check_modes(no, j.width, j.height, j.frames, j.matrix, j.range, &j.chroma, j.siting) != 0) return -1;
    if (!j.src || !j.dst) return no("src_yuv and dst_float4 must be device pointers");
    if (((uintptr_t)j.src | (uintptr_t)j.src_frame_stride) % 2 != 0) return no("src_yuv and src_frame_stride must be even (the samples are 16-bit)");
    const int64_t frame_bytes = mm_yuv10_frame_bytes(j.width, j.height), texel_bytes = (int64_t)j.width * j.height * 16;
    if (j.src_frame_stride < frame_bytes) return no(yuv_short_stride("src_frame_stride", j.src_frame_stride, "frame", frame_bytes));
    if ((uintptr_t)j.dst % 16 != 0) return no("dst_float4 is not 16-byte aligned (float4 texels)");
    if (j.dst_frame_stride % 16 != 0) return no("dst_frame_stride " + std::to_string(j.dst_frame_stride) + " is not a multiple of 16");
    if (j.dst_frame_stride < texel_bytes) return no(yuv_short_stride("dst_frame_stride", j.dst_frame_stride, "frame", texel_bytes));
    if (texel_bytes > ((int64_t)1 << 32)) return no("a destination frame of more than 4 GiB");
    return 0;
}

int launch_yuv420p10_to_float_clip(const YuvInJob &j, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err) {
    if (check_yuv420p10_to_float_clip(j, err) != 0) return -1;
    Yuv10InArgs a;
    a.src = (const uint16_t *)j.src;
    a.dst = (float *)j.dst;
    a.src_frame_samples = j.src_frame_stride / 2;
    a.dst_frame_stride = j.dst_frame_stride;
    a.cb_offset = (unsigned)mm_yuv_cb_offset(j.width, j.height);      // at most 2^28, a source frame at most 1.5 * 2^28 samples
    a.cr_offset = (unsigned)mm_yuv_cr_offset(j.width, j.height);
    a.width = (unsigned)j.width;
    a.height = (unsigned)j.height;
    a.cw = (unsigned)mm_yuv_cw(j.width);
    a.ch = (unsigned)mm_yuv_ch(j.height);
    a.m = MM_YUV10_FLOAT_MODES[j.matrix][j.range];
    // the aligned path: Y loads of up to 16 bytes at 2 * (row * width + 8 k), chroma loads of up to 8 bytes at 2 * (plane +
    // cy * width / 2 + 4 k): with the width a multiple of 8, 2 * width * height is a multiple of 16 and 2 * cw * ch one of 8
    const bool aligned = j.width % 8 == 0 && ((uintptr_t)j.src | (uintptr_t)j.src_frame_stride) % 16 == 0;
    // MMHIP_YUV10_IN_COLUMNS=2|4|8 and MMHIP_YUV10_IN_STORES=cached|nt, read per call: the A/Bs of tools/clip_yuv10_input_cost.py
    const unsigned cols = yuv_knob_is("MMHIP_YUV10_IN_COLUMNS", "8") ? 8u : yuv_knob_is("MMHIP_YUV10_IN_COLUMNS", "4") ? 4u : 2u;
    const bool nt = yuv_knob_is("MMHIP_YUV10_IN_STORES", "nt");
    const bool rep = j.chroma == MM_YUV_CHROMA_REPLICATE;
    a.per_pair = aligned ? a.width / cols : a.cw;
    a.items = a.per_pair * a.ch;
    const bool left = j.siting == MM_YUV_SITING_LEFT && !rep;      // replicate mode ignores the siting
    return yuv_launch(j.name, "yuv420p10_to_float_clip", a.items, j.frames, aligned, ws, s, path, err, [&](dim3 grid) {
        if (left && aligned && cols == 8) yuv10_in_launch_left<8>(nt, grid, s, a);
        else if (left && aligned && cols == 4) yuv10_in_launch_left<4>(nt, grid, s, a);
        else if (left && aligned) yuv10_in_launch_left<2>(nt, grid, s, a);
        else if (left) yuv10_in_launch_left<0>(nt, grid, s, a);
        else if (aligned && cols == 8) yuv10_in_launch<8>(rep, nt, grid, s, a);
        else if (aligned && cols == 4) yuv10_in_launch<4>(rep, nt, grid, s, a);
        else if (aligned) yuv10_in_launch<2>(rep, nt, grid, s, a);
        else yuv10_in_launch<0>(rep, nt, grid, s, a);
    });
}

}  // namespace mm
