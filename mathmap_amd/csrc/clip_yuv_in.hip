// Planar Y'CbCr 4:2:0 frames of a clip to the words of an input drawable (mmhip_clip_from_yuv420 in include/mmhip.h
// states the semantics, mm_yuv.h holds the arithmetic and the layout): the mirror image of clip_yuv.hip.  One launch over
// (tiles of a frame, frames), the frames in HBM on both sides.
#include <hip/hip_runtime.h>

#include "mm_yuv.h"
#include "clip_yuv_common.h"

namespace mm {

// Frame blockIdx.y of the call per grid row, 256 work-items per workgroup; a work-item owns whole 2 x 2 blocks, so no
// word of the output is written by two of them.  Offsets inside a frame are 32-bit from the frame's 64-bit bases, which
// are uniform over the workgroup: the launcher refuses a destination frame of more than 4 GiB (a source frame is 3/8 of
// it).
//   YUV_IN_WORDS  a work-item converts 8 columns of a row pair: one 8-byte Y load per row, one 4-byte load each of Cb and
//                 Cr, two 16-byte stores per row (a wave writes 2 KiB contiguous per row).  In bilinear mode it reads the
//                 chroma rows cy - 1 .. cy + 1 and, next to the four columns, the columns 4 at - 1 and 4 at + 4 with
//                 clamped byte loads (neighbours' cache lines: nothing is staged through LDS).  The launcher takes it
//                 where the width is a multiple of 8 and both sides are aligned for those accesses.
//   YUV_IN_BYTES  a work-item converts one 2 x 2 block with clamped byte loads and 4-byte stores: any width, height,
//                 pointer and stride.
// Both convert with mm_yuv.h's functions and give the same words.  The last row pair of an odd height has one row and the
// last block of an odd width one column: they are converted once and nothing is stored outside the frame.
struct YuvInArgs {
    const unsigned char *src;
    unsigned *dst;
    long long src_frame_stride, dst_frame_stride;      // bytes
    unsigned cb_offset, cr_offset;
    unsigned width, height, cw, ch;
    unsigned per_pair, items;      // work-items of a row pair and of a frame
    mm_yuv_rgba_mode m;
};

enum { YUV_IN_WORDS = 0, YUV_IN_BYTES = 1 };

// The column sums of one plane for one pixel row over the work-item's chroma columns 4 at .. 4 at + 3 and their
// neighbours: the pixel row's own chroma row `own` weighs 3, its neighbour row `nb` 1.  Centre siting takes six, 4 at - 1 ..
// 4 at + 4; left siting five, from 4 at on (below).  lo and hi are the clamped columns 4 at - 1 and 4 at + 4.
template <int SITING>
__device__ __forceinline__ void yuv_in_columns(const unsigned char *__restrict__ P, unsigned own, unsigned nb, unsigned at4, unsigned lo, unsigned hi,
                                               int *col) {
    constexpr int L = SITING == MM_YUV_SITING_LEFT ? 0 : 1;
    const unsigned a = *(const unsigned *)(P + (own + at4)), b = *(const unsigned *)(P + (nb + at4));
    if (L) col[0] = mm_yuv_chroma_column(P[own + lo], P[nb + lo]);
#pragma unroll
    for (int k = 0; k < 4; ++k) col[L + k] = mm_yuv_chroma_column((a >> (8 * k)) & 255u, (b >> (8 * k)) & 255u);
    col[L + 4] = mm_yuv_chroma_column(P[own + hi], P[nb + hi]);
}

// Eight pixels of one row: their luma bytes in y8, the chroma of pixel k in u[k], v[k].
template <bool NT>
__device__ __forceinline__ void yuv_in_row8(const mm_yuv_rgba_mode &m, yuv_u32x2 y8, const int u[8], const int v[8], unsigned *out) {
    yuv_u32x4 lo, hi;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo[k] = mm_yuv_to_rgba(m, (y8.x >> (8 * k)) & 255u, u[k], v[k]);
        hi[k] = mm_yuv_to_rgba(m, (y8.y >> (8 * k)) & 255u, u[4 + k], v[4 + k]);
    }
    yuv_store<NT>(lo, (yuv_u32x4 *)out);
    yuv_store<NT>(hi, (yuv_u32x4 *)out + 1);
}

// Left siting (SITING = MM_YUV_SITING_LEFT, bilinear mode only; mmhip_clip_from_yuv420_sited): an even pixel column lies
// on its chroma column and an odd one half way to the next, so a work-item needs its own chroma columns and the one to
// their right, 4 at + 4 clamped to the plane, and nothing to their left: five column sums per plane and pixel row where
// centre siting takes six.  Replicate mode ignores the siting: the launcher takes the centre instantiation for it.
template <int PATH, int CHROMA, bool NT, int SITING = MM_YUV_SITING_CENTER>
__global__ void __launch_bounds__(256) k_yuv420_to_rgba_clip(const YuvInArgs a) {
    constexpr bool LEFT = SITING == MM_YUV_SITING_LEFT;
    const unsigned item = yuv_item();
    if (item >= a.items) return;
    const unsigned cy = item / a.per_pair, at = item - cy * a.per_pair;      // cy < ch: items = per_pair * ch
    const unsigned r0 = 2u * cy;
    const bool two = r0 + 1u < a.height;
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ Y = a.src + fi * a.src_frame_stride;
    const unsigned char *__restrict__ CB = Y + a.cb_offset, *__restrict__ CR = Y + a.cr_offset;
    unsigned *__restrict__ D = (unsigned *)((unsigned char *)a.dst + fi * a.dst_frame_stride);
    const mm_yuv_rgba_mode m = a.m;
    // the chroma rows above and below, clamped to the plane: what the upper and the lower pixel row blend with
    const unsigned own = cy * a.cw, up = (cy ? cy - 1u : 0u) * a.cw, down = (cy + 1u < a.ch ? cy + 1u : cy) * a.cw;
    static_assert(!LEFT || CHROMA == MM_YUV_CHROMA_BILINEAR, "replicate mode has no siting");
    if (PATH == YUV_IN_WORDS) {
        const unsigned yo = r0 * a.width + at * 8u, at4 = at * 4u;      // below 2^30: a destination frame is at most 4 GiB
        const yuv_u32x2 y_top = *(const yuv_u32x2 *)(Y + yo);
        const yuv_u32x2 y_bot = two ? *(const yuv_u32x2 *)(Y + (yo + a.width)) : y_top;
        int u[8], v[8];
        if (CHROMA == MM_YUV_CHROMA_REPLICATE) {
            const unsigned cb = *(const unsigned *)(CB + (own + at4)), cr = *(const unsigned *)(CR + (own + at4));
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                u[k] = (cb >> (8 * (k >> 1))) & 255u;
                v[k] = (cr >> (8 * (k >> 1))) & 255u;
            }
            yuv_in_row8<NT>(m, y_top, u, v, D + yo);
            if (two) yuv_in_row8<NT>(m, y_bot, u, v, D + (yo + a.width));
            return;
        }
        const unsigned lo = at4 ? at4 - 1u : 0u, hi = at4 + 4u < a.cw ? at4 + 4u : a.cw - 1u;
        int cu[6], cv[6];
        if (LEFT) {
            // pixel k of the eight has its own column at index k / 2 of the five, an odd one its right neighbour one further
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j && !two) break;
                yuv_in_columns<SITING>(CB, own, j ? down : up, at4, lo, hi, cu);
                yuv_in_columns<SITING>(CR, own, j ? down : up, at4, lo, hi, cv);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    u[k] = mm_yuv_chroma_blend_left(cu[k >> 1], cu[(k >> 1) + 1], k & 1);
                    v[k] = mm_yuv_chroma_blend_left(cv[k >> 1], cv[(k >> 1) + 1], k & 1);
                }
                yuv_in_row8<NT>(m, j ? y_bot : y_top, u, v, D + (yo + (j ? a.width : 0u)));
            }
            return;
        }
        // pixel k of the eight has its own column at index 1 + k / 2 of the six, its neighbour one to the left (k even) or right
        yuv_in_columns<SITING>(CB, own, up, at4, lo, hi, cu);
        yuv_in_columns<SITING>(CR, own, up, at4, lo, hi, cv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = 1 + (k >> 1), n = (k & 1) ? c + 1 : c - 1;
            u[k] = mm_yuv_chroma_blend(cu[c], cu[n]);
            v[k] = mm_yuv_chroma_blend(cv[c], cv[n]);
        }
        yuv_in_row8<NT>(m, y_top, u, v, D + yo);
        if (!two) return;
        yuv_in_columns<SITING>(CB, own, down, at4, lo, hi, cu);
        yuv_in_columns<SITING>(CR, own, down, at4, lo, hi, cv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = 1 + (k >> 1), n = (k & 1) ? c + 1 : c - 1;
            u[k] = mm_yuv_chroma_blend(cu[c], cu[n]);
            v[k] = mm_yuv_chroma_blend(cv[c], cv[n]);
        }
        yuv_in_row8<NT>(m, y_bot, u, v, D + (yo + a.width));
        return;
    }
    // `at` is the chroma column: pixel columns 2 at and, inside the frame, 2 at + 1
    const unsigned c0 = 2u * at;
    const bool wide = c0 + 1u < a.width;
    const unsigned left = at ? at - 1u : 0u, right = at + 1u < a.cw ? at + 1u : at;
    const unsigned yo = r0 * a.width + c0;
    if (LEFT) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            const unsigned nb = j ? down : up;
            const int cu = mm_yuv_chroma_column(CB[own + at], CB[nb + at]), cv = mm_yuv_chroma_column(CR[own + at], CR[nb + at]);
            const unsigned o = yo + (j ? a.width : 0u);
            yuv_store<NT>((unsigned)mm_yuv_to_rgba(m, Y[o], mm_yuv_chroma_blend_left(cu, cu, 0), mm_yuv_chroma_blend_left(cv, cv, 0)), D + o);
            if (!wide) continue;
            const int ru = mm_yuv_chroma_column(CB[own + right], CB[nb + right]), rv = mm_yuv_chroma_column(CR[own + right], CR[nb + right]);
            yuv_store<NT>((unsigned)mm_yuv_to_rgba(m, Y[o + 1u], mm_yuv_chroma_blend_left(cu, ru, 1), mm_yuv_chroma_blend_left(cv, rv, 1)), D + (o + 1u));
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j && !two) break;
        const unsigned nb = j ? down : up;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i && !wide) break;
            int u, v;
            if (CHROMA == MM_YUV_CHROMA_REPLICATE) {
                u = CB[own + at];
                v = CR[own + at];
            } else {
                const unsigned nc = i ? right : left;
                u = mm_yuv_chroma_blend(mm_yuv_chroma_column(CB[own + at], CB[nb + at]), mm_yuv_chroma_column(CB[own + nc], CB[nb + nc]));
                v = mm_yuv_chroma_blend(mm_yuv_chroma_column(CR[own + at], CR[nb + at]), mm_yuv_chroma_column(CR[own + nc], CR[nb + nc]));
            }
            const unsigned o = yo + (j ? a.width : 0u) + (unsigned)i;
            yuv_store<NT>((unsigned)mm_yuv_to_rgba(m, Y[o], u, v), D + o);
        }
    }
}

template <int PATH, int CHROMA>
static void yuv_in_launch(bool nt, dim3 grid, hipStream_t s, const YuvInArgs &a) {
    if (nt) k_yuv420_to_rgba_clip<PATH, CHROMA, true><<<grid, 256, 0, s>>>(a);
    else k_yuv420_to_rgba_clip<PATH, CHROMA, false><<<grid, 256, 0, s>>>(a);
}
template <int PATH>
static void yuv_in_launch_left(bool nt, dim3 grid, hipStream_t s, const YuvInArgs &a) {
    if (nt) k_yuv420_to_rgba_clip<PATH, MM_YUV_CHROMA_BILINEAR, true, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
    else k_yuv420_to_rgba_clip<PATH, MM_YUV_CHROMA_BILINEAR, false, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
}

int check_yuv420_to_rgba_clip(const YuvInJob &j, std::string *err) {
    const YuvRefusal no(j.name, err);
    if (yuv_check_modes(no, j.width, j.height, j.frames, j.matrix, j.range, &j.chroma, j.siting) != 0) return -1;
    if (!j.src || !j.dst) return no("src_yuv and dst_rgba32 must be device pointers");
    const int64_t frame_bytes = mm_yuv_frame_bytes(j.width, j.height), words_bytes = (int64_t)j.width * j.height * 4;
    if (j.src_frame_stride < frame_bytes) return no(yuv_short_stride("src_frame_stride", j.src_frame_stride, "frame", frame_bytes));
    if (j.dst_frame_stride % 4 != 0) return no("dst_frame_stride " + std::to_string(j.dst_frame_stride) + " is not a multiple of 4");
    if (j.dst_frame_stride < words_bytes) return no(yuv_short_stride("dst_frame_stride", j.dst_frame_stride, "frame", words_bytes));
    if (words_bytes > ((int64_t)1 << 32)) return no("a destination frame of more than 4 GiB");
    return 0;
}

int launch_yuv420_to_rgba_clip(const YuvInJob &j, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err) {
    if (check_yuv420_to_rgba_clip(j, err) != 0) return -1;
    YuvInArgs a;
    a.src = (const unsigned char *)j.src;
    a.dst = (unsigned *)j.dst;
    a.src_frame_stride = j.src_frame_stride;
    a.dst_frame_stride = j.dst_frame_stride;
    a.cb_offset = (unsigned)mm_yuv_cb_offset(j.width, j.height);      // at most 2^30, a source frame at most 1.5 * 2^30
    a.cr_offset = (unsigned)mm_yuv_cr_offset(j.width, j.height);
    a.width = (unsigned)j.width;
    a.height = (unsigned)j.height;
    a.cw = (unsigned)mm_yuv_cw(j.width);
    a.ch = (unsigned)mm_yuv_ch(j.height);
    a.m = MM_YUV_RGBA_MODES[j.matrix][j.range];
    // YUV_IN_WORDS: 8-byte Y loads at row * width + 8 k, 4-byte chroma loads at plane + cy * width / 2 + 4 k (with the
    // width a multiple of 8, width * height is a multiple of 8 and both plane offsets multiples of 4), 16-byte stores at
    // 4 * (row * width + 8 k)
    const bool words = j.width % 8 == 0 && ((uintptr_t)j.src | (uintptr_t)j.src_frame_stride) % 8 == 0 &&
                       ((uintptr_t)j.dst | (uintptr_t)j.dst_frame_stride) % 16 == 0;
    a.per_pair = words ? a.width / 8u : a.cw;
    a.items = a.per_pair * a.ch;
    // MMHIP_YUV_IN_STORES=cached|nt, read per call: the A/B of tools/clip_yuv_input_cost.py
    const bool nt = yuv_knob_is("MMHIP_YUV_IN_STORES", "nt");
    const bool rep = j.chroma == MM_YUV_CHROMA_REPLICATE;
    const bool left = j.siting == MM_YUV_SITING_LEFT && !rep;      // replicate mode ignores the siting
    return yuv_launch(j.name, "yuv420_to_rgba_clip", a.items, j.frames, words, ws, s, path, err, [&](dim3 grid) {
        if (left && words) yuv_in_launch_left<YUV_IN_WORDS>(nt, grid, s, a);
        else if (left) yuv_in_launch_left<YUV_IN_BYTES>(nt, grid, s, a);
        else if (words && rep) yuv_in_launch<YUV_IN_WORDS, MM_YUV_CHROMA_REPLICATE>(nt, grid, s, a);
        else if (words) yuv_in_launch<YUV_IN_WORDS, MM_YUV_CHROMA_BILINEAR>(nt, grid, s, a);
        else if (rep) yuv_in_launch<YUV_IN_BYTES, MM_YUV_CHROMA_REPLICATE>(nt, grid, s, a);
        else yuv_in_launch<YUV_IN_BYTES, MM_YUV_CHROMA_BILINEAR>(nt, grid, s, a);
    });
}

}  // namespace mm
