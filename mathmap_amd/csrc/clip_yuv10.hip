// Float frames of a clip to planar Y'CbCr 4:2:0 with 10-bit samples (mmhip_clip_float_to_yuv420p10 in include/mmhip.h
// states the semantics, mm_yuv.h holds the arithmetic and the layout): clip_yuv.hip's sibling for the float maps every
// clip entry point lands with floatmap = 1.  One launch over (tiles of a frame's band, frames), the frames in HBM on both
// sides.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "mm_yuv.h"
#include "clip_kernels.h"

namespace mm {

// Frame blockIdx.y of the call per grid row, 256 work-items per workgroup; a work-item owns whole 2 x 2 chroma blocks, so
// no sample of the output is written by two of them.  Offsets inside a frame are 32-bit from the frame's 64-bit bases,
// which are uniform over the workgroup: byte offsets into the source band, sample offsets into the planes; the launcher
// refuses planes and source bands of more than 4 GiB.
//   COLS = 4 or 8  a work-item converts COLS columns of a row pair: per row COLS 16-byte loads of 16 * COLS contiguous bytes
//                  (a wave reads 4 or 8 KiB contiguous per row), one 8- or 16-byte Y store, and a 4- or 8-byte store each
//                  for Cb and Cr.  The launcher takes it where the width is a multiple of 8 and source and destination
//                  are aligned for 16-byte accesses.
//   COLS = 0       a work-item converts one 2 x 2 block with clamped per-pixel loads of three floats and 2-byte stores:
//                  any width, height, 4-byte aligned source and 2-byte aligned destination.
// All convert with mm_yuv.h's functions and give the same samples.  The last row pair of an odd height has one row: it
// is read twice (the replicated row) and its Y is stored once.  Everything is read once and written once: the stores are
// non-temporal like the other clip output stores; the loads are plain, because a lane's COLS loads of a row share cache
// lines with its neighbours' (a lane reads 64 or 128 bytes, an instruction 16 of them): non-temporal loads took 1.6 to 2.6
// times as long, and 8 columns were slower than 4 under either (profiles/r22_clip_yuv10_cost.json has both A/Bs).
struct Yuv10Args {
    const unsigned char *src;
    uint16_t *dst;
    long long src_frame_stride, dst_frame_samples, cb_offset, cr_offset;      // the last three in samples
    unsigned src_row_stride;
    unsigned width, height, cw, first_row;
    unsigned per_pair, items;      // work-items of a row pair and of a frame's band
    mm_yuv_mode m;
};

typedef float yuv10_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned yuv10_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned yuv10_u32x2 __attribute__((ext_vector_type(2)));

template <int WORDS> struct yuv10_words;
template <> struct yuv10_words<1> { typedef unsigned type; };
template <> struct yuv10_words<2> { typedef yuv10_u32x2 type; };
template <> struct yuv10_words<4> { typedef yuv10_u32x4 type; };

template <bool NT, class T>
__device__ __forceinline__ T yuv10_load(const T *p) {
    return NT ? __builtin_nontemporal_load(p) : *p;
}

// WORDS 32-bit words, two samples each (the even one low: little-endian), as one store
template <int WORDS>
__device__ __forceinline__ void yuv10_store(const unsigned *w, uint16_t *p) {
    typename yuv10_words<WORDS>::type v;
    if constexpr (WORDS == 1) v = w[0];
    else {
#pragma unroll
        for (int k = 0; k < WORDS; ++k) v[k] = w[k];
    }
    __builtin_nontemporal_store(v, (typename yuv10_words<WORDS>::type *)p);
}

// Left siting (SITING = MM_YUV_SITING_LEFT; mmhip_clip_float_to_yuv420p10_sited): a chroma sample weighs the pixel columns
// 2 cx - 1, 2 cx, 2 cx + 1 with 1, 2, 1, so a work-item needs the one pixel column left of its first block: one more
// 16-byte load per row, of the pixel at max(first column - 1, 0), out of the cache line its left neighbour reads whole
// (clamped load; the lane exchange was not built).  The aligned path has no right edge to clamp, COLS = 0 clamps the
// right column of an odd width's last block as centre siting does.  The matrix over the weighted sums ends 32 736 below
// 2^31, so mm_yuv10_chroma_left forms it in int64 (three 32 x 32 -> 64 multiply-adds).  Luma is the centre code's.
template <int COLS, bool NT, int SITING = MM_YUV_SITING_CENTER>
__global__ void __launch_bounds__(256) k_float_to_yuv420p10_clip(const Yuv10Args a) {
    const unsigned item = blockIdx.x * 256u + threadIdx.x;
    if (item >= a.items) return;
    const unsigned pair = item / a.per_pair, at = item - pair * a.per_pair;
    const unsigned r0 = a.first_row + 2u * pair;               // even; the band ends on an even row or on the frame's last
    const bool two = r0 + 1u < a.height;
    const unsigned s0 = 2u * pair * a.src_row_stride, s1 = two ? s0 + a.src_row_stride : s0;      // src is the band's first row
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ S = a.src + fi * a.src_frame_stride;
    uint16_t *__restrict__ Y = a.dst + fi * a.dst_frame_samples;
    uint16_t *__restrict__ CB = Y + a.cb_offset, *__restrict__ CR = Y + a.cr_offset;
    const mm_yuv_mode m = a.m;
    if constexpr (SITING == MM_YUV_SITING_LEFT && COLS != 0) {
        const yuv10_f32x4 *top = (const yuv10_f32x4 *)(S + (s0 + at * (16u * COLS))), *bot = (const yuv10_f32x4 *)(S + (s1 + at * (16u * COLS)));
        const unsigned lo = at ? at * (16u * COLS) - 16u : 0u;      // the pixel left of the first, or the first of the row
        yuv10_f32x4 t[COLS], b[COLS];
#pragma unroll
        for (int k = 0; k < COLS; ++k) t[k] = yuv10_load<NT>(top + k);
#pragma unroll
        for (int k = 0; k < COLS; ++k) b[k] = yuv10_load<NT>(bot + k);
        const yuv10_f32x4 lt = yuv10_load<NT>((const yuv10_f32x4 *)(S + (s0 + lo))), lb = yuv10_load<NT>((const yuv10_f32x4 *)(S + (s1 + lo)));
        unsigned yt[COLS / 2], yb[COLS / 2], cb[COLS / 4], cr[COLS / 4];
#pragma unroll
        for (int k = 0; k < COLS / 2; ++k) yt[k] = yb[k] = 0;
#pragma unroll
        for (int k = 0; k < COLS / 4; ++k) cb[k] = cr[k] = 0;
        int col[COLS + 1][3];      // pixel columns COLS at - 1 .. COLS at + COLS - 1: the sums of the two rows
        col[0][0] = mm_yuv10_quant(lt.x) + mm_yuv10_quant(lb.x);
        col[0][1] = mm_yuv10_quant(lt.y) + mm_yuv10_quant(lb.y);
        col[0][2] = mm_yuv10_quant(lt.z) + mm_yuv10_quant(lb.z);
#pragma unroll
        for (int k = 0; k < COLS; ++k) {
            const int tr = mm_yuv10_quant(t[k].x), tg = mm_yuv10_quant(t[k].y), tb = mm_yuv10_quant(t[k].z);
            const int br = mm_yuv10_quant(b[k].x), bg = mm_yuv10_quant(b[k].y), bb = mm_yuv10_quant(b[k].z);
            yt[k / 2] |= (unsigned)mm_yuv10_luma(m, tr, tg, tb) << (16 * (k & 1));
            yb[k / 2] |= (unsigned)mm_yuv10_luma(m, br, bg, bb) << (16 * (k & 1));
            col[1 + k][0] = tr + br;
            col[1 + k][1] = tg + bg;
            col[1 + k][2] = tb + bb;
        }
#pragma unroll
        for (int k = 0; k < COLS / 2; ++k) {      // one chroma sample
            const int rs = mm_yuv_left_sum(col[2 * k][0], col[2 * k + 1][0], col[2 * k + 2][0]);
            const int gs = mm_yuv_left_sum(col[2 * k][1], col[2 * k + 1][1], col[2 * k + 2][1]);
            const int bs = mm_yuv_left_sum(col[2 * k][2], col[2 * k + 1][2], col[2 * k + 2][2]);
            cb[k / 2] |= (unsigned)mm_yuv10_cb_left(m, rs, gs, bs) << (16 * (k & 1));
            cr[k / 2] |= (unsigned)mm_yuv10_cr_left(m, rs, gs, bs) << (16 * (k & 1));
        }
        const unsigned yo = r0 * a.width + at * COLS, co = (r0 >> 1) * a.cw + at * (COLS / 2);      // samples, below 2^31: a plane is at most 4 GiB
        yuv10_store<COLS / 2>(yt, Y + yo);
        if (two) yuv10_store<COLS / 2>(yb, Y + (yo + a.width));
        yuv10_store<COLS / 4>(cb, CB + co);
        yuv10_store<COLS / 4>(cr, CR + co);
    } else if constexpr (SITING == MM_YUV_SITING_LEFT) {
        // `at` is the chroma column: pixel columns 2 at - 1 (inside the frame), 2 at and, inside the frame, 2 at + 1
        const unsigned c0 = 2u * at;
        const bool wide = c0 + 1u < a.width;
        const unsigned c1 = wide ? c0 + 1u : c0, cl = at ? c0 - 1u : 0u;
        const unsigned src_off[6] = {s0 + c0 * 16u, s0 + c1 * 16u, s1 + c0 * 16u, s1 + c1 * 16u, s0 + cl * 16u, s1 + cl * 16u};
        int rs = 0, gs = 0, bs = 0, luma[4];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float *p = (const float *)(S + src_off[k]);
            const int r = mm_yuv10_quant(yuv10_load<NT>(p)), g = mm_yuv10_quant(yuv10_load<NT>(p + 1)), bl = mm_yuv10_quant(yuv10_load<NT>(p + 2));
            if (k < 4) luma[k] = mm_yuv10_luma(m, r, g, bl);
            const int weight = (k == 0 || k == 2) ? 2 : 1;      // the own column 2, its neighbours 1
            rs += weight * r;
            gs += weight * g;
            bs += weight * bl;
        }
        const unsigned yo = r0 * a.width + c0, co = (r0 >> 1) * a.cw + at;
        __builtin_nontemporal_store((uint16_t)luma[0], Y + yo);
        if (wide) __builtin_nontemporal_store((uint16_t)luma[1], Y + (yo + 1u));
        if (two) {
            __builtin_nontemporal_store((uint16_t)luma[2], Y + (yo + a.width));
            if (wide) __builtin_nontemporal_store((uint16_t)luma[3], Y + (yo + a.width + 1u));
        }
        __builtin_nontemporal_store((uint16_t)mm_yuv10_cb_left(m, rs, gs, bs), CB + co);
        __builtin_nontemporal_store((uint16_t)mm_yuv10_cr_left(m, rs, gs, bs), CR + co);
    } else if constexpr (COLS != 0) {
        const yuv10_f32x4 *top = (const yuv10_f32x4 *)(S + (s0 + at * (16u * COLS))), *bot = (const yuv10_f32x4 *)(S + (s1 + at * (16u * COLS)));
        yuv10_f32x4 t[COLS], b[COLS];
#pragma unroll
        for (int k = 0; k < COLS; ++k) t[k] = yuv10_load<NT>(top + k);
#pragma unroll
        for (int k = 0; k < COLS; ++k) b[k] = yuv10_load<NT>(bot + k);
        unsigned yt[COLS / 2], yb[COLS / 2], cb[COLS / 4], cr[COLS / 4];
#pragma unroll
        for (int k = 0; k < COLS / 2; ++k) yt[k] = yb[k] = 0;
#pragma unroll
        for (int k = 0; k < COLS / 4; ++k) cb[k] = cr[k] = 0;
#pragma unroll
        for (int k = 0; k < COLS; k += 2) {      // one 2 x 2 block
            int rs = 0, gs = 0, bs = 0;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int tr = mm_yuv10_quant(t[k + i].x), tg = mm_yuv10_quant(t[k + i].y), tb = mm_yuv10_quant(t[k + i].z);
                const int br = mm_yuv10_quant(b[k + i].x), bg = mm_yuv10_quant(b[k + i].y), bb = mm_yuv10_quant(b[k + i].z);
                yt[k / 2] |= (unsigned)mm_yuv10_luma(m, tr, tg, tb) << (16 * i);
                yb[k / 2] |= (unsigned)mm_yuv10_luma(m, br, bg, bb) << (16 * i);
                rs += tr + br;
                gs += tg + bg;
                bs += tb + bb;
            }
            cb[k / 4] |= (unsigned)mm_yuv10_cb(m, rs, gs, bs) << (16 * ((k / 2) & 1));
            cr[k / 4] |= (unsigned)mm_yuv10_cr(m, rs, gs, bs) << (16 * ((k / 2) & 1));
        }
        const unsigned yo = r0 * a.width + at * COLS, co = (r0 >> 1) * a.cw + at * (COLS / 2);      // samples, below 2^31: a plane is at most 4 GiB
        yuv10_store<COLS / 2>(yt, Y + yo);
        if (two) yuv10_store<COLS / 2>(yb, Y + (yo + a.width));
        yuv10_store<COLS / 4>(cb, CB + co);
        yuv10_store<COLS / 4>(cr, CR + co);
    } else {
        // `at` is the chroma column: pixel columns 2 at and, inside the frame, 2 at + 1
        const unsigned c0 = 2u * at;
        const bool wide = c0 + 1u < a.width;
        const unsigned c1 = wide ? c0 + 1u : c0;
        const unsigned src_off[4] = {s0 + c0 * 16u, s0 + c1 * 16u, s1 + c0 * 16u, s1 + c1 * 16u};
        int rs = 0, gs = 0, bs = 0, luma[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float *p = (const float *)(S + src_off[k]);
            const int r = mm_yuv10_quant(yuv10_load<NT>(p)), g = mm_yuv10_quant(yuv10_load<NT>(p + 1)), bl = mm_yuv10_quant(yuv10_load<NT>(p + 2));
            luma[k] = mm_yuv10_luma(m, r, g, bl);
            rs += r;
            gs += g;
            bs += bl;
        }
        const unsigned yo = r0 * a.width + c0, co = (r0 >> 1) * a.cw + at;
        __builtin_nontemporal_store((uint16_t)luma[0], Y + yo);
        if (wide) __builtin_nontemporal_store((uint16_t)luma[1], Y + (yo + 1u));
        if (two) {
            __builtin_nontemporal_store((uint16_t)luma[2], Y + (yo + a.width));
            if (wide) __builtin_nontemporal_store((uint16_t)luma[3], Y + (yo + a.width + 1u));
        }
        __builtin_nontemporal_store((uint16_t)mm_yuv10_cb(m, rs, gs, bs), CB + co);
        __builtin_nontemporal_store((uint16_t)mm_yuv10_cr(m, rs, gs, bs), CR + co);
    }
}

int check_float_to_yuv420p10_clip_sited(const char *name, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height,
                                        int first_row, int last_row, int frames, int matrix, int range, int siting, const void *dst,
                                        int64_t dst_frame_stride, std::string *err) {
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
    if (!src || !dst) return no("src and dst must be device pointers");
    if (src_row_stride < (int64_t)width * 16)
        return no("src_row_stride " + std::to_string(src_row_stride) + " is smaller than one row (" + std::to_string((int64_t)width * 16) + " bytes)");
    if (((uintptr_t)src | (uintptr_t)src_row_stride | (uintptr_t)src_frame_stride) % 4 != 0)
        return no("src, src_row_stride and src_frame_stride must be multiples of 4 (the source holds floats)");
    const int64_t frame_bytes = mm_yuv10_frame_bytes(width, height);
    if (dst_frame_stride < frame_bytes)
        return no("dst_frame_stride " + std::to_string(dst_frame_stride) + " is smaller than one frame (" + std::to_string(frame_bytes) + " bytes)");
    if (((uintptr_t)dst | (uintptr_t)dst_frame_stride) % 2 != 0) return no("dst and dst_frame_stride must be even (the samples are 16-bit)");
    if ((int64_t)width * height * 2 > ((int64_t)1 << 32)) return no("a Y plane of more than 4 GiB");
    if ((int64_t)(last_row - first_row - 1) * src_row_stride + (int64_t)width * 16 > ((int64_t)1 << 32))
        return no("a source frame of more than 4 GiB; convert the frame in row bands");
    return 0;
}

int check_float_to_yuv420p10_clip(const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height, int first_row,
                                  int last_row, int frames, int matrix, int range, const void *dst, int64_t dst_frame_stride, std::string *err) {
    return check_float_to_yuv420p10_clip_sited("clip_float_to_yuv420p10", src, src_row_stride, src_frame_stride, width, height, first_row, last_row,
                                               frames, matrix, range, MM_YUV_SITING_CENTER, dst, dst_frame_stride, err);
}

template <int SITING>
static void yuv10_launch(bool aligned, bool eight, bool nt, dim3 grid, hipStream_t s, const Yuv10Args &a) {
    if (aligned && eight && nt) k_float_to_yuv420p10_clip<8, true, SITING><<<grid, 256, 0, s>>>(a);
    else if (aligned && eight) k_float_to_yuv420p10_clip<8, false, SITING><<<grid, 256, 0, s>>>(a);
    else if (aligned && nt) k_float_to_yuv420p10_clip<4, true, SITING><<<grid, 256, 0, s>>>(a);
    else if (aligned) k_float_to_yuv420p10_clip<4, false, SITING><<<grid, 256, 0, s>>>(a);
    else if (nt) k_float_to_yuv420p10_clip<0, true, SITING><<<grid, 256, 0, s>>>(a);
    else k_float_to_yuv420p10_clip<0, false, SITING><<<grid, 256, 0, s>>>(a);
}

int launch_float_to_yuv420p10_clip_sited(const char *name, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height,
                                         int first_row, int last_row, int frames, int matrix, int range, int siting, void *dst,
                                         int64_t dst_frame_stride, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err) {
    if (check_float_to_yuv420p10_clip_sited(name, src, src_row_stride, src_frame_stride, width, height, first_row, last_row, frames, matrix, range,
                                            siting, dst, dst_frame_stride, err) != 0)
        return -1;
    Yuv10Args a;
    a.src = (const unsigned char *)src;
    a.dst = (uint16_t *)dst;
    a.src_frame_stride = src_frame_stride;
    a.dst_frame_samples = dst_frame_stride / 2;
    a.cb_offset = mm_yuv_cb_offset(width, height);
    a.cr_offset = mm_yuv_cr_offset(width, height);
    a.src_row_stride = (unsigned)src_row_stride;
    a.width = (unsigned)width;
    a.height = (unsigned)height;
    a.cw = (unsigned)mm_yuv_cw(width);
    a.first_row = (unsigned)first_row;
    a.m = MM_YUV10_MODES[matrix][range];
    const unsigned pairs = (unsigned)(last_row - first_row + 1) / 2u;
    // the aligned path: 16-byte loads; Y stores of up to 16 bytes at 2 * (row * width + 8 k), chroma stores of up to 8 bytes
    // at 2 * (plane + row * width / 2 + 4 k) (with the width a multiple of 8 both plane offsets are multiples of 8 bytes)
    const bool aligned = width % 8 == 0 && ((uintptr_t)src | (uintptr_t)src_row_stride | (uintptr_t)src_frame_stride) % 16 == 0 &&
                         ((uintptr_t)dst | (uintptr_t)dst_frame_stride) % 16 == 0;
    // MMHIP_YUV10_COLUMNS=4|8 and MMHIP_YUV10_LOADS=cached|nt, read per call: the A/Bs of tools/clip_yuv10_cost.py
    const char *columns = getenv("MMHIP_YUV10_COLUMNS"), *loads = getenv("MMHIP_YUV10_LOADS");
    const bool eight = columns && !strcmp(columns, "8");
    const bool nt = loads && !strcmp(loads, "nt");
    a.per_pair = aligned ? a.width / (eight ? 8u : 4u) : a.cw;
    a.items = a.per_pair * pairs;
    *path = aligned ? 0 : 1;
    const dim3 grid((a.items + 255u) / 256u, (unsigned)frames);
    ws.timed_launch("yuv420p10_clip", s, [&] {
        if (siting == MM_YUV_SITING_LEFT) yuv10_launch<MM_YUV_SITING_LEFT>(aligned, eight, nt, grid, s, a);
        else yuv10_launch<MM_YUV_SITING_CENTER>(aligned, eight, nt, grid, s, a);
    });
    if (hipGetLastError() != hipSuccess) {
        *err = std::string(name) + ": kernel launch failed";
        return -1;
    }
    return 0;
}

int launch_float_to_yuv420p10_clip(const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height, int first_row,
                                   int last_row, int frames, int matrix, int range, void *dst, int64_t dst_frame_stride, NativeWorkspace &ws,
                                   hipStream_t s, int *path, std::string *err) {
    return launch_float_to_yuv420p10_clip_sited("clip_float_to_yuv420p10", src, src_row_stride, src_frame_stride, width, height, first_row, last_row,
                                                frames, matrix, range, MM_YUV_SITING_CENTER, dst, dst_frame_stride, ws, s, path, err);
}

}  // namespace mm
