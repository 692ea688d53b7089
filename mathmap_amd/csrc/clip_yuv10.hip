// Float frames of a clip to planar Y'CbCr 4:2:0 with 10-bit samples (mmhip_clip_float_to_yuv420p10 in include/mmhip.h
// states the semantics, mm_yuv.h holds the arithmetic and the layout): clip_yuv.hip's sibling for the float maps every
// clip entry point lands with floatmap = 1.  One launch over (tiles of a frame's band, frames), the frames in HBM on both
// sides.
#include <hip/hip_runtime.h>

#include "mm_yuv.h"
#include "clip_yuv_common.h"

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

template <int WORDS> struct yuv10_words;
template <> struct yuv10_words<1> { typedef unsigned type; };
template <> struct yuv10_words<2> { typedef yuv_u32x2 type; };
template <> struct yuv10_words<4> { typedef yuv_u32x4 type; };

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
    constexpr bool LEFT = SITING == MM_YUV_SITING_LEFT;
    const unsigned item = yuv_item();
    if (item >= a.items) return;
    const YuvItem w = yuv_place(item, a.per_pair, a.first_row, a.height);
    const unsigned pair = w.pair, at = w.at, r0 = w.r0;
    const bool two = w.two;
    const unsigned s0 = 2u * pair * a.src_row_stride, s1 = two ? s0 + a.src_row_stride : s0;      // src is the band's first row
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ S = a.src + fi * a.src_frame_stride;
    uint16_t *__restrict__ Y = a.dst + fi * a.dst_frame_samples;
    uint16_t *__restrict__ CB = Y + a.cb_offset, *__restrict__ CR = Y + a.cr_offset;
    const mm_yuv_mode m = a.m;
    if constexpr (COLS != 0) {
        const yuv_f32x4 *top = (const yuv_f32x4 *)(S + (s0 + at * (16u * COLS))), *bot = (const yuv_f32x4 *)(S + (s1 + at * (16u * COLS)));
        yuv_f32x4 t[COLS], b[COLS];
#pragma unroll
        for (int k = 0; k < COLS; ++k) t[k] = yuv_load<NT>(top + k);
#pragma unroll
        for (int k = 0; k < COLS; ++k) b[k] = yuv_load<NT>(bot + k);
        unsigned yt[COLS / 2], yb[COLS / 2], cb[COLS / 4], cr[COLS / 4];
#pragma unroll
        for (int k = 0; k < COLS / 2; ++k) yt[k] = yb[k] = 0;
#pragma unroll
        for (int k = 0; k < COLS / 4; ++k) cb[k] = cr[k] = 0;
        if constexpr (LEFT) {
            const unsigned lo = at ? at * (16u * COLS) - 16u : 0u;      // the pixel left of the first, or the first of the row
            const yuv_f32x4 lt = yuv_load<NT>((const yuv_f32x4 *)(S + (s0 + lo))), lb = yuv_load<NT>((const yuv_f32x4 *)(S + (s1 + lo)));
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
        } else {
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
        }
        const unsigned yo = r0 * a.width + at * COLS, co = (r0 >> 1) * a.cw + at * (COLS / 2);      // samples, below 2^31: a plane is at most 4 GiB
        yuv10_store<COLS / 2>(yt, Y + yo);
        if (two) yuv10_store<COLS / 2>(yb, Y + (yo + a.width));
        yuv10_store<COLS / 4>(cb, CB + co);
        yuv10_store<COLS / 4>(cr, CR + co);
    } else {
        // `at` is the chroma column: pixel columns 2 at and, inside the frame, 2 at + 1; left siting adds 2 at - 1, inside the frame
        const unsigned c0 = 2u * at;
        const bool wide = c0 + 1u < a.width;
        const unsigned c1 = wide ? c0 + 1u : c0, cl = at ? c0 - 1u : 0u;
        const unsigned src_off[6] = {s0 + c0 * 16u, s0 + c1 * 16u, s1 + c0 * 16u, s1 + c1 * 16u, s0 + cl * 16u, s1 + cl * 16u};
        int rs = 0, gs = 0, bs = 0, luma[4];
#pragma unroll
        for (int k = 0; k < (LEFT ? 6 : 4); ++k) {
            const float *p = (const float *)(S + src_off[k]);
            const int r = mm_yuv10_quant(yuv_load<NT>(p)), g = mm_yuv10_quant(yuv_load<NT>(p + 1)), bl = mm_yuv10_quant(yuv_load<NT>(p + 2));
            if (k < 4) luma[k] = mm_yuv10_luma(m, r, g, bl);
            const int weight = LEFT && (k == 0 || k == 2) ? 2 : 1;      // left siting: the own column 2, its neighbours 1
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
        __builtin_nontemporal_store((uint16_t)(LEFT ? mm_yuv10_cb_left(m, rs, gs, bs) : mm_yuv10_cb(m, rs, gs, bs)), CB + co);
        __builtin_nontemporal_store((uint16_t)(LEFT ? mm_yuv10_cr_left(m, rs, gs, bs) : mm_yuv10_cr(m, rs, gs, bs)), CR + co);
    }
}

int check_float_to_yuv420p10_clip(const YuvOutJob &j, std::string *err) {
    const YuvRefusal no(j.name, err);
    if (yuv_check_modes(no, j.width, j.height, j.frames, j.matrix, j.range, nullptr, j.siting) != 0 || yuv_check_band(no, j) != 0) return -1;
    if (!j.src || !j.dst) return no("src and dst must be device pointers");
    if (j.src_row_stride < (int64_t)j.width * 16) return no(yuv_short_stride("src_row_stride", j.src_row_stride, "row", (int64_t)j.width * 16));
    if (((uintptr_t)j.src | (uintptr_t)j.src_row_stride | (uintptr_t)j.src_frame_stride) % 4 != 0)
        return no("src, src_row_stride and src_frame_stride must be multiples of 4 (the source holds floats)");
    const int64_t frame_bytes = mm_yuv10_frame_bytes(j.width, j.height);
    if (j.dst_frame_stride < frame_bytes) return no(yuv_short_stride("dst_frame_stride", j.dst_frame_stride, "frame", frame_bytes));
    if (((uintptr_t)j.dst | (uintptr_t)j.dst_frame_stride) % 2 != 0) return no("dst and dst_frame_stride must be even (the samples are 16-bit)");
    if ((int64_t)j.width * j.height * 2 > ((int64_t)1 << 32)) return no("a Y plane of more than 4 GiB");
    if ((int64_t)(j.last_row - j.first_row - 1) * j.src_row_stride + (int64_t)j.width * 16 > ((int64_t)1 << 32))
        return no("a source frame of more than 4 GiB; convert the frame in row bands");
    return 0;
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

int launch_float_to_yuv420p10_clip(const YuvOutJob &j, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err) {
    if (check_float_to_yuv420p10_clip(j, err) != 0) return -1;
    Yuv10Args a;
    a.src = (const unsigned char *)j.src;
    a.dst = (uint16_t *)j.dst;
    a.src_frame_stride = j.src_frame_stride;
    a.dst_frame_samples = j.dst_frame_stride / 2;
    a.cb_offset = mm_yuv_cb_offset(j.width, j.height);
    a.cr_offset = mm_yuv_cr_offset(j.width, j.height);
    a.src_row_stride = (unsigned)j.src_row_stride;
    a.width = (unsigned)j.width;
    a.height = (unsigned)j.height;
    a.cw = (unsigned)mm_yuv_cw(j.width);
    a.first_row = (unsigned)j.first_row;
    a.m = MM_YUV10_MODES[j.matrix][j.range];
    const unsigned pairs = (unsigned)(j.last_row - j.first_row + 1) / 2u;
    // the aligned path: 16-byte loads; Y stores of up to 16 bytes at 2 * (row * width + 8 k), chroma stores of up to 8 bytes
    // at 2 * (plane + row * width / 2 + 4 k) (with the width a multiple of 8 both plane offsets are multiples of 8 bytes)
    const bool aligned = j.width % 8 == 0 && ((uintptr_t)j.src | (uintptr_t)j.src_row_stride | (uintptr_t)j.src_frame_stride) % 16 == 0 &&
                         ((uintptr_t)j.dst | (uintptr_t)j.dst_frame_stride) % 16 == 0;
    // MMHIP_YUV10_COLUMNS=4|8 and MMHIP_YUV10_LOADS=cached|nt, read per call: the A/Bs of tools/clip_yuv10_cost.py
    const bool eight = yuv_knob_is("MMHIP_YUV10_COLUMNS", "8"), nt = yuv_knob_is("MMHIP_YUV10_LOADS", "nt");
    a.per_pair = aligned ? a.width / (eight ? 8u : 4u) : a.cw;
    a.items = a.per_pair * pairs;
    return yuv_launch(j.name, "yuv420p10_clip", a.items, j.frames, aligned, ws, s, path, err, [&](dim3 grid) {
        if (j.siting == MM_YUV_SITING_LEFT) yuv10_launch<MM_YUV_SITING_LEFT>(aligned, eight, nt, grid, s, a);
        else yuv10_launch<MM_YUV_SITING_CENTER>(aligned, eight, nt, grid, s, a);
    });
}

}  // namespace mm
