// RGBA8 frames of a clip to planar Y'CbCr 4:2:0 (mmhip_clip_to_yuv420 in include/mmhip.h states the semantics,
// mm_yuv.h holds the arithmetic and the layout): one launch over (tiles of a frame, frames), the frames in HBM on both
// sides.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "mm_yuv.h"
#include "clip_kernels.h"

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

typedef unsigned yuv_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned yuv_u32x2 __attribute__((ext_vector_type(2)));

enum { YUV_WORDS = 0, YUV_BYTES = 1 };

template <bool NT, class T>
__device__ __forceinline__ T yuv_load(const T *p) {
    return NT ? __builtin_nontemporal_load(p) : *p;
}

// Four pixels of both rows of a row pair: their four luma bytes of each row packed into a word, and the sums of the two
// 2 x 2 blocks.
__device__ __forceinline__ void yuv_four(const mm_yuv_mode &m, yuv_u32x4 top, yuv_u32x4 bot, unsigned *y_top, unsigned *y_bot, int sums[2][3]) {
    unsigned yt = 0, yb = 0;
    for (int k = 0; k < 2; ++k) sums[k][0] = sums[k][1] = sums[k][2] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tr = top[k] & 255u, tg = (top[k] >> 8) & 255u, tb = (top[k] >> 16) & 255u;
        const int br = bot[k] & 255u, bg = (bot[k] >> 8) & 255u, bb = (bot[k] >> 16) & 255u;
        yt |= (unsigned)mm_yuv_luma(m, tr, tg, tb) << (8 * k);
        yb |= (unsigned)mm_yuv_luma(m, br, bg, bb) << (8 * k);
        sums[k >> 1][0] += tr + br;
        sums[k >> 1][1] += tg + bg;
        sums[k >> 1][2] += tb + bb;
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

// Four pixels of both rows of a row pair: their four luma bytes of each row packed into a word, and per pixel column the
// sums of the two rows.
__device__ __forceinline__ void yuv_four_columns(const mm_yuv_mode &m, yuv_u32x4 top, yuv_u32x4 bot, unsigned *y_top, unsigned *y_bot, int col[4][3]) {
    unsigned yt = 0, yb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int tr = top[k] & 255u, tg = (top[k] >> 8) & 255u, tb = (top[k] >> 16) & 255u;
        const int br = bot[k] & 255u, bg = (bot[k] >> 8) & 255u, bb = (bot[k] >> 16) & 255u;
        yt |= (unsigned)mm_yuv_luma(m, tr, tg, tb) << (8 * k);
        yb |= (unsigned)mm_yuv_luma(m, br, bg, bb) << (8 * k);
        col[k][0] = tr + br;
        col[k][1] = tg + bg;
        col[k][2] = tb + bb;
    }
    *y_top = yt;
    *y_bot = yb;
}

template <int PATH, bool NT, int SITING = MM_YUV_SITING_CENTER>
__global__ void __launch_bounds__(256) k_rgba8_to_yuv420_clip(const YuvArgs a) {
    const unsigned item = blockIdx.x * 256u + threadIdx.x;
    if (item >= a.items) return;
    const unsigned pair = item / a.per_pair, at = item - pair * a.per_pair;
    const unsigned r0 = a.first_row + 2u * pair;               // even; the band ends on an even row or on the frame's last
    const bool two = r0 + 1u < a.height;
    const unsigned s0 = 2u * pair * a.src_row_stride, s1 = two ? s0 + a.src_row_stride : s0;      // src is the band's first row
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ S = a.src + fi * a.src_frame_stride;
    unsigned char *__restrict__ Y = a.dst + fi * a.dst_frame_stride;
    unsigned char *__restrict__ CB = Y + a.cb_offset, *__restrict__ CR = Y + a.cr_offset;
    const mm_yuv_mode m = a.m;
    if constexpr (SITING == MM_YUV_SITING_LEFT) {
        if (PATH == YUV_WORDS) {
            const yuv_u32x4 *top = (const yuv_u32x4 *)(S + (s0 + at * 32u)), *bot = (const yuv_u32x4 *)(S + (s1 + at * 32u));
            const unsigned lo = at ? at * 32u - 4u : 0u;      // the pixel left of the first, or the first of the row
            const yuv_u32x4 t0 = yuv_load<NT>(top), t1 = yuv_load<NT>(top + 1), b0 = yuv_load<NT>(bot), b1 = yuv_load<NT>(bot + 1);
            const unsigned lt = yuv_load<NT>((const unsigned *)(S + (s0 + lo))), lb = yuv_load<NT>((const unsigned *)(S + (s1 + lo)));
            yuv_u32x2 yt, yb;
            unsigned w0, w1;
            int col[9][3];      // pixel columns 8 at - 1 .. 8 at + 7
            col[0][0] = (int)((lt & 255u) + (lb & 255u));
            col[0][1] = (int)(((lt >> 8) & 255u) + ((lb >> 8) & 255u));
            col[0][2] = (int)(((lt >> 16) & 255u) + ((lb >> 16) & 255u));
            yuv_four_columns(m, t0, b0, &w0, &w1, col + 1);
            yt.x = w0;
            yb.x = w1;
            yuv_four_columns(m, t1, b1, &w0, &w1, col + 5);
            yt.y = w0;
            yb.y = w1;
            unsigned cb = 0, cr = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int rs = mm_yuv_left_sum(col[2 * k][0], col[2 * k + 1][0], col[2 * k + 2][0]);
                const int gs = mm_yuv_left_sum(col[2 * k][1], col[2 * k + 1][1], col[2 * k + 2][1]);
                const int bs = mm_yuv_left_sum(col[2 * k][2], col[2 * k + 1][2], col[2 * k + 2][2]);
                cb |= (unsigned)mm_yuv_cb_left(m, rs, gs, bs) << (8 * k);
                cr |= (unsigned)mm_yuv_cr_left(m, rs, gs, bs) << (8 * k);
            }
            const unsigned yo = r0 * a.width + at * 8u, co = (r0 >> 1) * a.cw + at * 4u;      // below 2^32: a plane is at most 4 GiB
            __builtin_nontemporal_store(yt, (yuv_u32x2 *)(Y + yo));
            if (two) __builtin_nontemporal_store(yb, (yuv_u32x2 *)(Y + (yo + a.width)));
            __builtin_nontemporal_store(cb, (unsigned *)(CB + co));
            __builtin_nontemporal_store(cr, (unsigned *)(CR + co));
            return;
        }
        // `at` is the chroma column: pixel columns 2 at - 1 (inside the frame), 2 at and, inside the frame, 2 at + 1
        const unsigned c0 = 2u * at;
        const bool wide = c0 + 1u < a.width;
        const unsigned c1 = wide ? c0 + 1u : c0, cl = at ? c0 - 1u : 0u;
        const unsigned src_off[6] = {s0 + c0 * 4u, s0 + c1 * 4u, s1 + c0 * 4u, s1 + c1 * 4u, s0 + cl * 4u, s1 + cl * 4u};
        int rs = 0, gs = 0, bs = 0, luma[4];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const unsigned char *p = S + src_off[k];
            const int r = yuv_load<NT>(p), g = yuv_load<NT>(p + 1), b = yuv_load<NT>(p + 2);
            if (k < 4) luma[k] = mm_yuv_luma(m, r, g, b);
            const int weight = (k == 0 || k == 2) ? 2 : 1;      // the own column 2, its neighbours 1
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
        __builtin_nontemporal_store((unsigned char)mm_yuv_cb_left(m, rs, gs, bs), CB + co);
        __builtin_nontemporal_store((unsigned char)mm_yuv_cr_left(m, rs, gs, bs), CR + co);
        return;
    }
    if (PATH == YUV_WORDS) {
        const yuv_u32x4 *top = (const yuv_u32x4 *)(S + (s0 + at * 32u)), *bot = (const yuv_u32x4 *)(S + (s1 + at * 32u));
        const yuv_u32x4 t0 = yuv_load<NT>(top), t1 = yuv_load<NT>(top + 1), b0 = yuv_load<NT>(bot), b1 = yuv_load<NT>(bot + 1);
        yuv_u32x2 yt, yb;
        unsigned w0, w1;
        int lo[2][3], hi[2][3];
        yuv_four(m, t0, b0, &w0, &w1, lo);
        yt.x = w0;
        yb.x = w1;
        yuv_four(m, t1, b1, &w0, &w1, hi);
        yt.y = w0;
        yb.y = w1;
        const unsigned cb = (unsigned)mm_yuv_cb(m, lo[0][0], lo[0][1], lo[0][2]) | (unsigned)mm_yuv_cb(m, lo[1][0], lo[1][1], lo[1][2]) << 8 |
                            (unsigned)mm_yuv_cb(m, hi[0][0], hi[0][1], hi[0][2]) << 16 | (unsigned)mm_yuv_cb(m, hi[1][0], hi[1][1], hi[1][2]) << 24;
        const unsigned cr = (unsigned)mm_yuv_cr(m, lo[0][0], lo[0][1], lo[0][2]) | (unsigned)mm_yuv_cr(m, lo[1][0], lo[1][1], lo[1][2]) << 8 |
                            (unsigned)mm_yuv_cr(m, hi[0][0], hi[0][1], hi[0][2]) << 16 | (unsigned)mm_yuv_cr(m, hi[1][0], hi[1][1], hi[1][2]) << 24;
        const unsigned yo = r0 * a.width + at * 8u, co = (r0 >> 1) * a.cw + at * 4u;      // below 2^32: a plane is at most 4 GiB
        __builtin_nontemporal_store(yt, (yuv_u32x2 *)(Y + yo));
        if (two) __builtin_nontemporal_store(yb, (yuv_u32x2 *)(Y + (yo + a.width)));
        __builtin_nontemporal_store(cb, (unsigned *)(CB + co));
        __builtin_nontemporal_store(cr, (unsigned *)(CR + co));
        return;
    }
    // `at` is the chroma column: pixel columns 2 at and, inside the frame, 2 at + 1
    const unsigned c0 = 2u * at;
    const bool wide = c0 + 1u < a.width;
    const unsigned c1 = wide ? c0 + 1u : c0;
    const unsigned src_off[4] = {s0 + c0 * 4u, s0 + c1 * 4u, s1 + c0 * 4u, s1 + c1 * 4u};
    int rs = 0, gs = 0, bs = 0, luma[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned char *p = S + src_off[k];
        const int r = yuv_load<NT>(p), g = yuv_load<NT>(p + 1), b = yuv_load<NT>(p + 2);
        luma[k] = mm_yuv_luma(m, r, g, b);
        rs += r;
        gs += g;
        bs += b;
    }
    const unsigned yo = r0 * a.width + c0, co = (r0 >> 1) * a.cw + at;
    __builtin_nontemporal_store((unsigned char)luma[0], Y + yo);
    if (wide) __builtin_nontemporal_store((unsigned char)luma[1], Y + (yo + 1u));
    if (two) {
        __builtin_nontemporal_store((unsigned char)luma[2], Y + (yo + a.width));
        if (wide) __builtin_nontemporal_store((unsigned char)luma[3], Y + (yo + a.width + 1u));
    }
    __builtin_nontemporal_store((unsigned char)mm_yuv_cb(m, rs, gs, bs), CB + co);
    __builtin_nontemporal_store((unsigned char)mm_yuv_cr(m, rs, gs, bs), CR + co);
}

int check_rgba8_to_yuv420_clip_sited(const char *name, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height,
                                     int first_row, int last_row, int frames, int matrix, int range, int siting, const void *dst,
                                     int64_t dst_frame_stride, std::string *err) {
    (void)src_frame_stride;
    const std::string who = std::string(name) + ": ";
    auto no = [&](const std::string &what) {
        *err = who + what;
        return -1;
    };
    if (width < 1 || height < 1) return no("width and height must be at least 1, not " + std::to_string(width) + " x " + std::to_string(height));
    if (frames < 1) return no("num_frames must be at least 1");
    if (frames > 65535) return no("more than 65535 frames in one call (" + std::to_string(frames) + "); convert the clip in groups");
    if (matrix < 0 || matrix >= MM_YUV_MATRICES) return no("matrix must be MMHIP_YUV_BT601 or MMHIP_YUV_BT709 (0 or 1), not " + std::to_string(matrix));
    if (range < 0 || range >= MM_YUV_RANGES) return no("range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not " + std::to_string(range));
    if (!mm_yuv_siting_known(siting))
        return no("siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not " + std::to_string(siting));
    if (first_row < 0 || last_row > height || first_row >= last_row)
        return no("rows [" + std::to_string(first_row) + ", " + std::to_string(last_row) + ") are not rows of a frame of " + std::to_string(height));
    if (first_row & 1) return no("first_row must be even, not " + std::to_string(first_row));
    if ((last_row & 1) && last_row != height)
        return no("last_row must be even or equal to height, not " + std::to_string(last_row) + " of " + std::to_string(height));
    if (!src || !dst) return no("src_rgba and dst must be device pointers");
    if (src_row_stride < (int64_t)width * 4)
        return no("src_row_stride " + std::to_string(src_row_stride) + " is smaller than one row (" + std::to_string((int64_t)width * 4) + " bytes)");
    const int64_t frame_bytes = mm_yuv_frame_bytes(width, height);
    if (dst_frame_stride < frame_bytes)
        return no("dst_frame_stride " + std::to_string(dst_frame_stride) + " is smaller than one frame (" + std::to_string(frame_bytes) + " bytes)");
    if ((int64_t)width * height > ((int64_t)1 << 32)) return no("a Y plane of more than 4 GiB");
    if ((int64_t)(last_row - first_row - 1) * src_row_stride + (int64_t)width * 4 > ((int64_t)1 << 32))
        return no("a source frame of more than 4 GiB; convert the frame in row bands");
    return 0;
}

int check_rgba8_to_yuv420_clip(const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height, int first_row,
                               int last_row, int frames, int matrix, int range, const void *dst, int64_t dst_frame_stride, std::string *err) {
    return check_rgba8_to_yuv420_clip_sited("clip_to_yuv420", src, src_row_stride, src_frame_stride, width, height, first_row, last_row, frames, matrix,
                                            range, MM_YUV_SITING_CENTER, dst, dst_frame_stride, err);
}

int launch_rgba8_to_yuv420_clip_sited(const char *name, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height,
                                      int first_row, int last_row, int frames, int matrix, int range, int siting, void *dst,
                                      int64_t dst_frame_stride, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err) {
    if (check_rgba8_to_yuv420_clip_sited(name, src, src_row_stride, src_frame_stride, width, height, first_row, last_row, frames, matrix, range, siting,
                                         dst, dst_frame_stride, err) != 0)
        return -1;
    YuvArgs a;
    a.src = (const unsigned char *)src;
    a.dst = (unsigned char *)dst;
    a.src_frame_stride = src_frame_stride;
    a.dst_frame_stride = dst_frame_stride;
    a.cb_offset = mm_yuv_cb_offset(width, height);
    a.cr_offset = mm_yuv_cr_offset(width, height);
    a.src_row_stride = (unsigned)src_row_stride;
    a.width = (unsigned)width;
    a.height = (unsigned)height;
    a.cw = (unsigned)mm_yuv_cw(width);
    a.first_row = (unsigned)first_row;
    a.m = MM_YUV_MODES[matrix][range];
    const unsigned pairs = (unsigned)(last_row - first_row + 1) / 2u;
    // YUV_WORDS: 16-byte loads, 8-byte Y stores at row * width + 8 k, 4-byte chroma stores at plane + row * width / 2 + 4 k
    // (with the width a multiple of 8 both plane offsets are multiples of 4)
    const bool words = width % 8 == 0 && ((uintptr_t)src | (uintptr_t)src_row_stride | (uintptr_t)src_frame_stride) % 16 == 0 &&
                       ((uintptr_t)dst | (uintptr_t)dst_frame_stride) % 8 == 0;
    a.per_pair = words ? a.width / 8u : a.cw;
    a.items = a.per_pair * pairs;
    // MMHIP_YUV_LOADS=cached|nt, read per call: the A/B of tools/clip_yuv_cost.py
    const char *loads = getenv("MMHIP_YUV_LOADS");
    const bool nt = !(loads && !strcmp(loads, "cached"));
    const dim3 grid((a.items + 255u) / 256u, (unsigned)frames);
    const bool left = siting == MM_YUV_SITING_LEFT;
    ws.timed_launch("yuv420_clip", s, [&] {
        if (left && words && nt) k_rgba8_to_yuv420_clip<YUV_WORDS, true, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
        else if (left && words) k_rgba8_to_yuv420_clip<YUV_WORDS, false, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
        else if (left && nt) k_rgba8_to_yuv420_clip<YUV_BYTES, true, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
        else if (left) k_rgba8_to_yuv420_clip<YUV_BYTES, false, MM_YUV_SITING_LEFT><<<grid, 256, 0, s>>>(a);
        else if (words && nt) k_rgba8_to_yuv420_clip<YUV_WORDS, true><<<grid, 256, 0, s>>>(a);
        else if (words) k_rgba8_to_yuv420_clip<YUV_WORDS, false><<<grid, 256, 0, s>>>(a);
        else if (nt) k_rgba8_to_yuv420_clip<YUV_BYTES, true><<<grid, 256, 0, s>>>(a);
        else k_rgba8_to_yuv420_clip<YUV_BYTES, false><<<grid, 256, 0, s>>>(a);
    });
    if (hipGetLastError() != hipSuccess) {
        *err = std::string(name) + ": kernel launch failed";
        return -1;
    }
    if (path) *path = words ? YUV_WORDS : YUV_BYTES;
    return 0;
}

int launch_rgba8_to_yuv420_clip(const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height, int first_row,
                                int last_row, int frames, int matrix, int range, void *dst, int64_t dst_frame_stride, NativeWorkspace &ws,
                                hipStream_t s, std::string *err) {
    return launch_rgba8_to_yuv420_clip_sited("clip_to_yuv420", src, src_row_stride, src_frame_stride, width, height, first_row, last_row, frames,
                                             matrix, range, MM_YUV_SITING_CENTER, dst, dst_frame_stride, ws, s, nullptr, err);
}

}  // namespace mm
