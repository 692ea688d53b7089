// RGBA8 frames of a clip to planar Y'CbCr 4:2:0 (mmhip_clip_to_yuv420 in include/mmhip.h states the semantics,
// mm_yuv.h holds the arithmetic and the layout): one launch over (tiles of a frame, frames), the frames in HBM on both
// sides.
#include <hip/hip_runtime.h>

#include "mm_yuv.h"
#include "clip_yuv_common.h"

namespace mm {

// Frame blockIdx.y of the call per grid row, 256 work-items per workgroup; a work-item owns whole 2 x 2 chroma blocks, so
// no byte of the output is written by two of them.  Offsets inside a frame are 32-bit from the frame's 64-bit bases,
// which are uniform over the workgroup: the launcher refuses planes and source bands of more than 4 GiB.
//   YUV_WORDS  a work-item converts 8 columns of a row pair: per row 32 bytes in two 16-byte loads (a wave reads 2 KiB
//              contiguous per row) and one 8-byte Y store, one 4-byte store each for Cb and Cr.  The launcher takes it
//              where the width is a multiple of 8 and source and destination are aligned for those accesses.
//   YUV_BYTES  a work-item converts one 2 x 2 block with clamped per-pixel byte loads and byte stores: any width, height,
//              pointer and stride.
// Both convert with mm_yuv.h's two functions and give the same bytes.  The last row pair of an odd height has one row:
// it is read twice (the replicated row) and its Y is stored once.  Everything is read once and written once: the stores
// are non-temporal like the other clip output stores, the loads with NT (profiles/r18_clip_yuv_cost.json has the A/B).
struct YuvArgs {
    const unsigned char *src;
    unsigned char *dst;
    long long src_frame_stride, dst_frame_stride, cb_offset, cr_offset;
    unsigned src_row_stride;
    unsigned width, height, cw, first_row;
    unsigned per_pair, items;      // work-items of a row pair and of a frame's band
    mm_yuv_mode m;
};

enum { YUV_WORDS = 0, YUV_BYTES = 1 };

// Four pixels of both rows of a row pair: their four luma bytes of each row packed into a word, and the sums of the two
// rows over every PER pixel columns: the two 2 x 2 blocks (PER = 2) or the four columns (PER = 1).
template <int PER>
__device__ __forceinline__ void yuv_four(const mm_yuv_mode &m, yuv_u32x4 top, yuv_u32x4 bot, unsigned *y_top, unsigned *y_bot, int sums[4 / PER][3]) {
    unsigned yt = 0, yb = 0;
    for (int k = 0; k < 4 / PER; ++k) sums[k][0] = sums[k][1] = sums[k][2] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tr = top[k] & 255u, tg = (top[k] >> 8) & 255u, tb = (top[k] >> 16) & 255u;
        const int br = bot[k] & 255u, bg = (bot[k] >> 8) & 255u, bb = (bot[k] >> 16) & 255u;
        yt |= (unsigned)mm_yuv_luma(m, tr, tg, tb) << (8 * k);
        yb |= (unsigned)mm_yuv_luma(m, br, bg, bb) << (8 * k);
        sums[k / PER][0] += tr + br;
        sums[k / PER][1] += tg + bg;
        sums[k / PER][2] += tb + bb;
    }
    *y_top = yt;
    *y_bot = yb;
}

// Left siting (SITING = MM_YUV_SITING_LEFT; mmhip_clip_to_yuv420_sited): a chroma sample weighs the pixel columns 2 cx - 1,
// 2 cx, 2 cx + 1 with 1, 2, 1, so a work-item needs the one pixel column left of its first block next to its own -- its
// last block's right column is its own.  It takes it with one more load per row, of the pixel at max(first column - 1, 0):
// a clamped load of 4 bytes out of the cache line its left neighbour reads whole (the neighbouring lane holds the pixel
// too, but a wave's first lane and a row's first work-item need the load anyway; the lane exchange was not built, so
// nothing was measured against it).  YUV_WORDS has no right edge to clamp (the width is a multiple of 8), YUV_BYTES
// clamps the right column of an odd width's last block as centre siting does.  Luma is the centre code's.
template <int PATH, bool NT, int SITING = MM_YUV_SITING_CENTER>
__global__ void __launch_bounds__(256) k_rgba8_to_yuv420_clip(const YuvArgs a) {
    constexpr bool LEFT = SITING == MM_YUV_SITING_LEFT;
    const unsigned item = yuv_item();
    if (item >= a.items) return;
    const YuvItem w = yuv_place(item, a.per_pair, a.first_row, a.height);
    const unsigned pair = w.pair, at = w.at, r0 = w.r0;
    const bool two = w.two;
    const unsigned s0 = 2u * pair * a.src_row_stride, s1 = two ? s0 + a.src_row_stride : s0;      // src is the band's first row
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ S = a.src + fi * a.src_frame_stride;
    unsigned char *__restrict__ Y = a.dst + fi * a.dst_frame_stride;
    unsigned char *__restrict__ CB = Y + a.cb_offset, *__restrict__ CR = Y + a.cr_offset;
    const mm_yuv_mode m = a.m;
    if (PATH == YUV_WORDS) {
        const yuv_u32x4 *top = (const yuv_u32x4 *)(S + (s0 + at * 32u)), *bot = (const yuv_u32x4 *)(S + (s1 + at * 32u));
        const yuv_u32x4 t0 = yuv_load<NT>(top), t1 = yuv_load<NT>(top + 1), b0 = yuv_load<NT>(bot), b1 = yuv_load<NT>(bot + 1);
        yuv_u32x2 yt, yb;
        unsigned w0, w1;
        unsigned cb = 0, cr = 0;
        if (LEFT) {
            const unsigned lo = at ? at * 32u - 4u : 0u;      // the pixel left of the first, or the first of the row
            const unsigned lt = yuv_load<NT>((const unsigned *)(S + (s0 + lo))), lb = yuv_load<NT>((const unsigned *)(S + (s1 + lo)));
            int col[9][3];      // pixel columns 8 at - 1 .. 8 at + 7
            col[0][0] = (int)((lt & 255u) + (lb & 255u));
            col[0][1] = (int)(((lt >> 8) & 255u) + ((lb >> 8) & 255u));
            col[0][2] = (int)(((lt >> 16) & 255u) + ((lb >> 16) & 255u));
            yuv_four<1>(m, t0, b0, &w0, &w1, col + 1);
            yt.x = w0;
            yb.x = w1;
            yuv_four<1>(m, t1, b1, &w0, &w1, col + 5);
            yt.y = w0;
            yb.y = w1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int rs = mm_yuv_left_sum(col[2 * k][0], col[2 * k + 1][0], col[2 * k + 2][0]);
                const int gs = mm_yuv_left_sum(col[2 * k][1], col[2 * k + 1][1], col[2 * k + 2][1]);
                const int bs = mm_yuv_left_sum(col[2 * k][2], col[2 * k + 1][2], col[2 * k + 2][2]);
                cb |= (unsigned)mm_yuv_cb_left(m, rs, gs, bs) << (8 * k);
                cr |= (unsigned)mm_yuv_cr_left(m, rs, gs, bs) << (8 * k);
            }
        } else {
            int lo[2][3], hi[2][3];      // the sums of the four 2 x 2 blocks
            yuv_four<2>(m, t0, b0, &w0, &w1, lo);
            yt.x = w0;
            yb.x = w1;
            yuv_four<2>(m, t1, b1, &w0, &w1, hi);
            yt.y = w0;
            yb.y = w1;
            cb = (unsigned)mm_yuv_cb(m, lo[0][0], lo[0][1], lo[0][2]) | (unsigned)mm_yuv_cb(m, lo[1][0], lo[1][1], lo[1][2]) << 8 |
                 (unsigned)mm_yuv_cb(m, hi[0][0], hi[0][1], hi[0][2]) << 16 | (unsigned)mm_yuv_cb(m, hi[1][0], hi[1][1], hi[1][2]) << 24;
            cr = (unsigned)mm_yuv_cr(m, lo[0][0], lo[0][1], lo[0][2]) | (unsigned)mm_yuv_cr(m, lo[1][0], lo[1][1], lo[1][2]) << 8 |
                 (unsigned)mm_yuv_cr(m, hi[0][0], hi[0][1], hi[0][2]) << 16 | (unsigned)mm_yuv_cr(m, hi[1][0], hi[1][1], hi[1][2]) << 24;
        }
        const unsigned yo = r0 * a.width + at * 8u, co = (r0 >> 1) * a.cw + at * 4u;      // below 2^32: a plane is at most 4 GiB
        __builtin_nontemporal_store(yt, (yuv_u32x2 *)(Y + yo));
        if (two) __builtin_nontemporal_store(yb, (yuv_u32x2 *)(Y + (yo + a.width)));
        __builtin_nontemporal_store(cb, (unsigned *)(CB + co));
        __builtin_nontemporal_store(cr, (unsigned *)(CR + co));
        return;
    }
    // `at` is the chroma column: pixel columns 2 at and, inside the frame, 2 at + 1; left siting adds 2 at - 1, inside the frame
    const unsigned c0 = 2u * at;
    const bool wide = c0 + 1u < a.width;
    const unsigned c1 = wide ? c0 + 1u : c0, cl = at ? c0 - 1u : 0u;
    const unsigned src_off[6] = {s0 + c0 * 4u, s0 + c1 * 4u, s1 + c0 * 4u, s1 + c1 * 4u, s0 + cl * 4u, s1 + cl * 4u};
    int rs = 0, gs = 0, bs = 0, luma[4];
#pragma unroll
    for (int k = 0; k < (LEFT ? 6 : 4); ++k) {
        const unsigned char *p = S + src_off[k];
        const int r = yuv_load<NT>(p), g = yuv_load<NT>(p + 1), b = yuv_load<NT>(p + 2);
        if (k < 4) luma[k] = mm_yuv_luma(m, r, g, b);
        const int weight = LEFT && (k == 0 || k == 2) ? 2 : 1;      // left siting: the own column 2, its neighbours 1
        rs += weight * r;
        gs += weight * g;
        bs += weight * b;
    }
    const unsigned yo = r0 * a.width + c0, co = (r0 >> 1) * a.cw + at;
    __builtin_nontemporal_store((unsigned char)luma[0], Y + yo);
    if (wide) __builtin_nontemporal_store((unsigned char)luma[1], Y + (yo + 1u));
    if (two) {
        __builtin_nontemporal_store((unsigned char)luma[2], Y + (yo + a.width));
        if (wide) __builtin_nontemporal_store((unsigned char)luma[3], Y + (yo + a.width + 1u));
    }
    __builtin_nontemporal_store((unsigned char)(LEFT ? mm_yuv_cb_left(m, rs, gs, bs) : mm_yuv_cb(m, rs, gs, bs)), CB + co);
    __builtin_nontemporal_store((unsigned char)(LEFT ? mm_yuv_cr_left(m, rs, gs, bs) : mm_yuv_cr(m, rs, gs, bs)), CR + co);
}

int check_rgba8_to_yuv420_clip(const YuvOutJob &j, std::string *err) {
    const YuvRefusal no(j.name, err);
    if (yuv_check_modes(no, j.width, j.height, j.frames, j.matrix, j.range, nullptr, j.siting) != 0 || yuv_check_band(no, j) != 0) return -1;
    if (!j.src || !j.dst) return no("src_rgba and dst must be device pointers");
    if (j.src_row_stride < (int64_t)j.width * 4) return no(yuv_short_stride("src_row_stride", j.src_row_stride, "row", (int64_t)j.width * 4));
    const int64_t frame_bytes = mm_yuv_frame_bytes(j.width, j.height);
    if (j.dst_frame_stride < frame_bytes) return no(yuv_short_stride("dst_frame_stride", j.dst_frame_stride, "frame", frame_bytes));
    if ((int64_t)j.width * j.height > ((int64_t)1 << 32)) return no("a Y plane of more than 4 GiB");
    if ((int64_t)(j.last_row - j.first_row - 1) * j.src_row_stride + (int64_t)j.width * 4 > ((int64_t)1 << 32))
        return no("a source frame of more than 4 GiB; convert the frame in row bands");
    return 0;
}

int launch_rgba8_to_yuv420_clip(const YuvOutJob &j, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err) {
    if (check_rgba8_to_yuv420_clip(j, err) != 0) return -1;
    YuvArgs a;
    a.src = (const unsigned char *)j.src;
    a.dst = (unsigned char *)j.dst;
    a.src_frame_stride = j.src_frame_stride;
    a.dst_frame_stride = j.dst_frame_stride;
    a.cb_offset = mm_yuv_cb_offset(j.width, j.height);
    a.cr_offset = mm_yuv_cr_offset(j.width, j.height);
    a.src_row_stride = (unsigned)j.src_row_stride;
    a.width = (unsigned)j.width;
    a.height = (unsigned)j.height;
    a.cw = (unsigned)mm_yuv_cw(j.width);
    a.first_row = (unsigned)j.first_row;
    a.m = MM_YUV_MODES[j.matrix][j.range];
    const unsigned pairs = (unsigned)(j.last_row - j.first_row + 1) / 2u;
    // YUV_WORDS: 16-byte loads, 8-byte Y stores at row * width + 8 k, 4-byte chroma stores at plane + row * width / 2 + 4 k
    // (with the width a multiple of 8 both plane offsets are multiples of 4)
    const bool words = j.width % 8 == 0 && ((uintptr_t)j.src | (uintptr_t)j.src_row_stride | (uintptr_t)j.src_frame_stride) % 16 == 0 &&
                       ((uintptr_t)j.dst | (uintptr_t)j.dst_frame_stride) % 8 == 0;
    a.per_pair = words ? a.width / 8u : a.cw;
    a.items = a.per_pair * pairs;
    // MMHIP_YUV_LOADS=cached|nt, read per call: the A/B of tools/clip_yuv_cost.py
    const bool nt = !yuv_knob_is("MMHIP_YUV_LOADS", "cached");
    const bool left = j.siting == MM_YUV_SITING_LEFT;
    return yuv_launch(j.name, "yuv420_clip", a.items, j.frames, words, ws, s, path, err, [&](dim3 grid) {
        if (left && words && nt) k_rgba8_to_yuv420_clip<YUV_WORDS, true, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
        else if (left && words) k_rgba8_to_yuv420_clip<YUV_WORDS, false, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
        else if (left && nt) k_rgba8_to_yuv420_clip<YUV_BYTES, true, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
        else if (left) k_rgba8_to_yuv420_clip<YUV_BYTES, false, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
        else if (words && nt) k_rgba8_to_yuv420_clip<YUV_WORDS, true><<<grid, 256, 0, s>>>(a);
        else if (words) k_rgba8_to_yuv420_clip<YUV_WORDS, false><<<grid, 256, 0, s>>>(a);
        else if (nt) k_rgba8_to_yuv420_clip<YUV_BYTES, true><<<grid, 256, 0, s>>>(a);
        else k_rgba8_to_yuv420_clip<YUV_BYTES, false><<<grid, 256, 0, s>>>(a);
    });
}

}  // namespace mm
