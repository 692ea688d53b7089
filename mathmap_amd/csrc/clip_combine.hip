// The hand-written kernels that finish a clip, for gfx950: the supersampling combine (single-frame and clip), the
// shutter combine, the contrast mask of adaptive anti-aliasing and the reconstruction filter.  clip_kernels.h declares
// their launchers.  Compiled without floating-point contraction, like the headers that hold their arithmetic ask.
#include "clip_kernels.h"
#include "mm_clip_filter.h"
#include "mm_sample_grid.h"
#include "mm_shutter_combine.h"
#include "mm_ss_combine.h"
#include "pack_rgba8.h"

#include <algorithm>
#include <type_traits>

namespace mm {

// Supersampling combine of call_invocation (mathmap_common.c:880-927): per output byte
// (l1[c] + l1[c+1] + 2*l2[c] + l3[c] + l3[c+1]) / 6 in integer arithmetic, where l1/l3 are
// rows r and r+1 of the "long" slice (width+1, offset -0.5) and l2 row r of the short slice.
__global__ void __launch_bounds__(256) k_supersample_combine(const unsigned char *__restrict__ longs,
                                                             const unsigned char *__restrict__ shorts,
                                                             unsigned char *__restrict__ out, int w, int h, int bpp,
                                                             int out_stride) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)w * h * bpp) return;
    const int b = (int)(i % bpp);
    const long px = i / bpp;
    const int col = (int)(px % w), row = (int)(px / w);
    const long lstride = (long)(w + 1) * bpp;
    const unsigned char *l1 = longs + row * lstride;
    // the reference's last iteration renders no new line3 (calc_lines clips at the slice end),
    // so line3 still equals line1 there
    const unsigned char *l3 = longs + (row + 1 < h ? row + 1 : row) * lstride;
    const unsigned char *l2 = shorts + (long)row * w * bpp;
    const int v = (l1[col * bpp + b] + l1[(col + 1) * bpp + b] + 2 * l2[col * bpp + b] + l3[col * bpp + b] +
                   l3[(col + 1) * bpp + b]) / 6;
    out[(long)row * out_stride + (long)col * bpp + b] = (unsigned char)v;
}

void launch_supersample_combine(const unsigned char *longs, const unsigned char *shorts, unsigned char *out, int w, int h,
                                int bpp, int out_stride, hipStream_t s) {
    const long n = (long)w * h * bpp;
    k_supersample_combine<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(longs, shorts, out, w, h, bpp, out_stride);
}

// ---- the combine over the frames of a supersampled clip (mmhip_render_clip_supersampled) ----
// The same bytes as k_supersample_combine, frame blockIdx.y of a batch per grid row.  A work-item owns SS_CLIP_PIXELS
// adjacent pixels (a column group) over a strip of SS_CLIP_ROWS rows; blockIdx.x counts the items of one frame, column
// groups fastest, so that a wave reads and writes runs of adjacent bytes.  The long slices' rows are long_pitch (a
// multiple of 16) bytes apart, the short slices' rows are packed.
struct SsClipArgs {
    const unsigned char *longs, *shorts;
    unsigned char *out;
    long long long_frame, short_frame, frame_stride;      // bytes from a frame to the next
    unsigned long_pitch, short_pitch;
    int row_stride;
    int w, h;
    unsigned groups, items;                               // column groups of a row; work-items of a frame
};

typedef uint32_t ss_u32x4 __attribute__((ext_vector_type(4)));
typedef ss_u32x4 ss_u32x4_a4 __attribute__((aligned(4)));      // a short row's group: dword-aligned only

// Pair sums of the group's four pixels from texels 4g .. 4g + 4 of a long row: the aligned 16 bytes and the texel behind them.
__device__ __forceinline__ void ss_long_sums(const unsigned char *row, bool fifth, mm_ss_halves sums[4]) {
    const ss_u32x4 v = *(const ss_u32x4 *)row;
    const uint32_t f = fifth ? *(const uint32_t *)(row + 16) : 0u;
    sums[0] = mm_ss_pair_sum(v.x, v.y);
    sums[1] = mm_ss_pair_sum(v.y, v.z);
    sums[2] = mm_ss_pair_sum(v.z, v.w);
    sums[3] = mm_ss_pair_sum(v.w, f);
}

// bpp 4, output dword-aligned (STORE16: 16-byte aligned, one store per row).  A long row is read once per strip (and
// the strip's first row once more): the pair sums of row r + 1 stay in registers for row r + 1's own turn.
template <bool STORE16>
__global__ void __launch_bounds__(256) k_supersample_combine_clip(const SsClipArgs a) {
    const unsigned item = blockIdx.x * 256u + threadIdx.x;
    if (item >= a.items) return;
    const unsigned strip = item / a.groups, g = item - strip * a.groups;
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ L = a.longs + fi * a.long_frame + (size_t)g * 16;
    const unsigned char *__restrict__ S = a.shorts + fi * a.short_frame + (size_t)g * 16;
    unsigned char *__restrict__ O = a.out + fi * a.frame_stride + (size_t)g * 16;
    const int r0 = (int)strip * SS_CLIP_ROWS;
    const int real = min(4, a.w - (int)g * 4);            // the last group of a row may hold 1 - 3 pixels
    mm_ss_halves top[4], bot[4];
    if (real == 4 && r0 + SS_CLIP_ROWS < a.h) {           // a whole group, and every row has a row below it
        ss_long_sums(L + (size_t)r0 * a.long_pitch, true, top);
#pragma unroll
        for (int i = 0; i < SS_CLIP_ROWS; ++i) {
            const int r = r0 + i;
            ss_long_sums(L + (size_t)(r + 1) * a.long_pitch, true, bot);
            const ss_u32x4 m = *(const ss_u32x4_a4 *)(S + (size_t)r * a.short_pitch);
            ss_u32x4 o;
            o.x = mm_ss_combine_word(top[0], bot[0], m.x);
            o.y = mm_ss_combine_word(top[1], bot[1], m.y);
            o.z = mm_ss_combine_word(top[2], bot[2], m.z);
            o.w = mm_ss_combine_word(top[3], bot[3], m.w);
            unsigned char *dst = O + (long long)r * a.row_stride;
            if (STORE16) __builtin_nontemporal_store(o, (ss_u32x4 *)dst);
            else
                for (int k = 0; k < 4; ++k) __builtin_nontemporal_store(o[k], (uint32_t *)dst + k);
            for (int k = 0; k < 4; ++k) top[k] = bot[k];
        }
        return;
    }
    // the frame's last strip and the row's last group: rows end at h (the last row's line3 is its line1, see
    // k_supersample_combine), only `real` pixels are read from the short row and stored, and the texel behind the
    // aligned 16 bytes is read only where the fourth pixel is real (the bytes of the 16 that no pixel launch wrote
    // feed sums of pixels that are not stored)
    const int r_end = min(r0 + SS_CLIP_ROWS, a.h);
    ss_long_sums(L + (size_t)r0 * a.long_pitch, real == 4, top);
    for (int r = r0; r < r_end; ++r) {
        if (r + 1 < a.h) ss_long_sums(L + (size_t)(r + 1) * a.long_pitch, real == 4, bot);
        else
            for (int k = 0; k < 4; ++k) bot[k] = top[k];
        const uint32_t *mid = (const uint32_t *)(S + (size_t)r * a.short_pitch);
        uint32_t *dst = (uint32_t *)(O + (long long)r * a.row_stride);
        for (int k = 0; k < 4; ++k)
            if (k < real) __builtin_nontemporal_store(mm_ss_combine_word(top[k], bot[k], mid[k]), dst + k);
        for (int k = 0; k < 4; ++k) top[k] = bot[k];
    }
}

// Any bpp and any output alignment, byte by byte over the same grid (the rare path).
template <int BPP>
__global__ void __launch_bounds__(256) k_supersample_combine_clip_bytes(const SsClipArgs a) {
    const unsigned item = blockIdx.x * 256u + threadIdx.x;
    if (item >= a.items) return;
    const unsigned strip = item / a.groups, g = item - strip * a.groups;
    const size_t fi = blockIdx.y;
    const size_t col0 = (size_t)g * SS_CLIP_PIXELS * BPP;
    const unsigned char *__restrict__ L = a.longs + fi * a.long_frame + col0;
    const unsigned char *__restrict__ S = a.shorts + fi * a.short_frame + col0;
    unsigned char *__restrict__ O = a.out + fi * a.frame_stride + col0;
    const int r0 = (int)strip * SS_CLIP_ROWS, r_end = min(r0 + SS_CLIP_ROWS, a.h);
    const int bytes = min(SS_CLIP_PIXELS, a.w - (int)g * SS_CLIP_PIXELS) * BPP;
    for (int r = r0; r < r_end; ++r) {
        const unsigned char *l1 = L + (size_t)r * a.long_pitch;
        const unsigned char *l3 = L + (size_t)(r + 1 < a.h ? r + 1 : r) * a.long_pitch;
        const unsigned char *l2 = S + (size_t)r * a.short_pitch;
        unsigned char *dst = O + (long long)r * a.row_stride;
        for (int b = 0; b < bytes; ++b)
            dst[b] = (unsigned char)mm_ss_div6((uint32_t)l1[b] + l1[b + BPP] + 2u * l2[b] + l3[b] + l3[b + BPP]);
    }
}

size_t supersample_clip_long_pitch(int w, int bpp) { return ((size_t)(w + 1) * bpp + 15) / 16 * 16; }

int64_t supersample_clip_items(int w, int h) {
    return (int64_t)((w + SS_CLIP_PIXELS - 1) / SS_CLIP_PIXELS) * ((h + SS_CLIP_ROWS - 1) / SS_CLIP_ROWS);
}

int launch_supersample_combine_clip(const unsigned char *longs, const unsigned char *shorts, unsigned char *out, int w, int h,
                                    int bpp, int row_stride, int64_t frame_stride, int frames, NativeWorkspace &ws, hipStream_t s,
                                    std::string *err) {
    const int64_t items = supersample_clip_items(w, h);
    const size_t long_pitch = supersample_clip_long_pitch(w, bpp);
    if (items > 0x7fffffffLL || long_pitch > 0x7fffffffULL || frames < 1 || frames > 65535) {
        *err = "supersample combine: the batch does not fit one launch";
        return -1;
    }
    SsClipArgs a;
    a.longs = longs;
    a.shorts = shorts;
    a.out = out;
    a.long_pitch = (unsigned)long_pitch;
    a.short_pitch = (unsigned)w * bpp;
    a.long_frame = (long long)h * (long long)long_pitch;
    a.short_frame = (long long)h * a.short_pitch;
    a.frame_stride = frame_stride;
    a.row_stride = row_stride;
    a.w = w;
    a.h = h;
    a.groups = (unsigned)((w + SS_CLIP_PIXELS - 1) / SS_CLIP_PIXELS);
    a.items = (unsigned)items;
    const dim3 grid((unsigned)((items + 255) / 256), (unsigned)frames);
    const uintptr_t align = (uintptr_t)out | (uintptr_t)row_stride | (uintptr_t)frame_stride;
    ws.timed_launch("supersample_combine_clip", s, [&] {
        if (bpp == 4 && align % 16 == 0) k_supersample_combine_clip<true><<<grid, 256, 0, s>>>(a);
        else if (bpp == 4 && align % 4 == 0) k_supersample_combine_clip<false><<<grid, 256, 0, s>>>(a);
        else if (bpp == 4) k_supersample_combine_clip_bytes<4><<<grid, 256, 0, s>>>(a);
        else if (bpp == 3) k_supersample_combine_clip_bytes<3><<<grid, 256, 0, s>>>(a);
        else if (bpp == 2) k_supersample_combine_clip_bytes<2><<<grid, 256, 0, s>>>(a);
        else k_supersample_combine_clip_bytes<1><<<grid, 256, 0, s>>>(a);
    });
    if (hipGetLastError() != hipSuccess) { *err = "supersample combine: kernel launch failed"; return -1; }
    return 0;
}

// ---- the temporal combine over the frames of a motion-blurred clip (mmhip_render_clip_shutter) ----
// Frame blockIdx.y of a batch per grid row, one pixel of the region per lane: blockIdx.x counts the region's pixels row
// by row, so a wave reads 1 KiB of adjacent float4 from every sub-sample map (but where it crosses a row end of a region
// narrower than the render width).  The one division is 32-bit and per work-item; a frame's maps are addressed by a
// 32-bit byte offset from wave-uniform bases that advance by sample_stride, and the sample loop is unrolled by four
// with the four loads ahead of the four sums.  Everything is read once and written once: non-temporal, but for the
// store of the carry map, which the next pass reads back.
struct ShutterArgs {
    const unsigned char *samples;
    unsigned char *carry_in, *carry_out, *out;            // (a pass may read and write one carry map: a lane owns its pixel)
    long long sample_stride, frame_samples_stride, carry_frame_stride, frame_stride;
    int row_stride, count;
    unsigned region_w, render_w, items;                   // items: region_w * rows, the work-items of a frame
    float inv_k;
};

typedef float sh_f32x4 __attribute__((ext_vector_type(4)));
typedef sh_f32x4 sh_f32x4_a4 __attribute__((aligned(4)));      // a float-map output: dword-aligned only

// How a kernel of this file leaves a pixel's mean (the MODE of the shutter combine, the contrast mask and the filter
// combine): a float map, the pixel store's bytes at output_bpp 1 - 4 (the mode is the bpp), or one 32-bit word per pixel
// at bpp 4.  CLIP_CARRY is the one mode that stores no pixel: the pass leaves its running sum in the carry map.
enum { CLIP_STORE_FLOATMAP = 0, CLIP_STORE_BYTES1 = 1, CLIP_STORE_BYTES2 = 2, CLIP_STORE_BYTES3 = 3, CLIP_STORE_BYTES4 = 4, CLIP_STORE_WORDS = 5, CLIP_CARRY = 6 };

__device__ __forceinline__ sh_f32x4 shutter_add(sh_f32x4 acc, sh_f32x4 f) {
    sh_f32x4 r;
    r.x = mm_shutter_add(acc.x, f.x);
    r.y = mm_shutter_add(acc.y, f.y);
    r.z = mm_shutter_add(acc.z, f.z);
    r.w = mm_shutter_add(acc.w, f.w);
    return r;
}

// The pixel store of the three kernels: the mean acc * inv_k of the pixel at (row, col) of the output rectangle, into
// frame fi of the batch at out + fi * frame_stride.  A float map takes it at map_off(), the pixel's byte offset in a map of
// the render width (a callable, so that a kernel which has no such offset yet forms it here, behind the scale); the pixel
// store's formats at row * row_stride + col * bpp.  `row` arrives as the caller extended it.
template <int MODE, bool NONTEMPORAL, class MapOff>
__device__ __forceinline__ void clip_store_mean(sh_f32x4 acc, float inv_k, unsigned char *out, size_t fi, long long frame_stride,
                                                MapOff map_off, long long row, int row_stride, unsigned col) {
    static_assert(MODE >= CLIP_STORE_FLOATMAP && MODE <= CLIP_STORE_WORDS, "a store mode");
    sh_f32x4 m;
    m.x = mm_shutter_scale(acc.x, inv_k);
    m.y = mm_shutter_scale(acc.y, inv_k);
    m.z = mm_shutter_scale(acc.z, inv_k);
    m.w = mm_shutter_scale(acc.w, inv_k);
    unsigned char *__restrict__ O = out + fi * frame_stride;
    if (MODE == CLIP_STORE_FLOATMAP) {
        sh_f32x4_a4 *p = (sh_f32x4_a4 *)(O + map_off());
        if (NONTEMPORAL) __builtin_nontemporal_store(m, p);
        else *p = m;
        return;
    }
    const int bpp = MODE == CLIP_STORE_WORDS ? 4 : MODE;
    unsigned char *p = O + row * row_stride + col * (unsigned)bpp;
    if (MODE != CLIP_STORE_WORDS) mm_shutter_store_bytes(p, m.x, m.y, m.z, m.w, bpp);
    else if (NONTEMPORAL) __builtin_nontemporal_store(pack_rgba8(make_float4(m.x, m.y, m.z, m.w)), (unsigned *)p);
    else *(unsigned *)p = pack_rgba8(make_float4(m.x, m.y, m.z, m.w));
}

template <int MODE>
__global__ void __launch_bounds__(256) k_shutter_combine_clip(const ShutterArgs a) {
    const unsigned item = blockIdx.x * 256u + threadIdx.x;
    if (item >= a.items) return;
    const unsigned row = item / a.region_w, col = item - row * a.region_w;
    const unsigned off = (row * a.render_w + col) * 16u;      // below 2^32: the launcher refuses larger maps
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ S = a.samples + fi * a.frame_samples_stride;
    sh_f32x4 acc;
    int j = 0;
    if (a.carry_in) acc = __builtin_nontemporal_load((const sh_f32x4 *)(a.carry_in + fi * a.carry_frame_stride + off));
    else {
        acc = __builtin_nontemporal_load((const sh_f32x4 *)(S + off));
        S += a.sample_stride;
        j = 1;
    }
    for (; j + 4 <= a.count; j += 4) {
        const sh_f32x4 f0 = __builtin_nontemporal_load((const sh_f32x4 *)(S + off));
        const sh_f32x4 f1 = __builtin_nontemporal_load((const sh_f32x4 *)(S + a.sample_stride + off));
        const sh_f32x4 f2 = __builtin_nontemporal_load((const sh_f32x4 *)(S + 2 * a.sample_stride + off));
        const sh_f32x4 f3 = __builtin_nontemporal_load((const sh_f32x4 *)(S + 3 * a.sample_stride + off));
        acc = shutter_add(shutter_add(shutter_add(shutter_add(acc, f0), f1), f2), f3);
        S += 4 * a.sample_stride;
    }
    for (; j < a.count; ++j) {
        acc = shutter_add(acc, __builtin_nontemporal_load((const sh_f32x4 *)(S + off)));
        S += a.sample_stride;
    }
    if constexpr (MODE == CLIP_CARRY) *(sh_f32x4 *)(a.carry_out + fi * a.carry_frame_stride + off) = acc;
    else clip_store_mean<MODE, true>(acc, a.inv_k, a.out, fi, a.frame_stride, [off] { return off; }, (long long)row, a.row_stride, col);
}

// ---- what the launchers of the three kernels share ----
// The mode a launch stores in: `carry` is the pass that leaves its sum in the carry map.
static int clip_store_mode(const ClipStore &to, bool carry) {
    const uintptr_t align = (uintptr_t)to.out | (uintptr_t)to.row_stride | (uintptr_t)to.frame_stride;
    return carry ? CLIP_CARRY : to.floatmap ? CLIP_STORE_FLOATMAP : to.bpp == 4 && align % 4 == 0 ? CLIP_STORE_WORDS : to.bpp;
}

// Calls launch(std::integral_constant<int, MODE>) for the mode of the enumeration that `mode` is.
template <int MODE = 0, class F>
static void with_store_mode(int mode, F &&launch) {
    if (mode == MODE) launch(std::integral_constant<int, MODE>{});
    else if constexpr (MODE < CLIP_CARRY) with_store_mode<MODE + 1>(mode, launch);
}

static bool clip_maps_aligned(const ClipSamples &in) {
    return ((uintptr_t)in.samples | (uintptr_t)in.sample_stride | (uintptr_t)in.frame_samples_stride | (uintptr_t)in.carry_in |
            (uintptr_t)in.carry_out) % 16 == 0;
}

// The refusals of a launch under the launcher's name `who`, in their order: a batch that does not fit one launch (the
// limits all three share, and `fits`: the caller's own), the caller's own refusal `also` (its text, or null), float maps
// that are not aligned (`maps_aligned`: the caller's inputs; a float-map output that a pass without `carry` stores to).
// map_bytes: one input map's.  Returns 0, or -1 with the text in *err.
static int check_clip_launch(const char *who, const ClipStore &to, bool carry, int region_w, int rows, int frames, int64_t map_bytes, bool fits,
                             const char *also, bool maps_aligned, std::string *err) {
    const char *what = nullptr;
    if (region_w < 1 || rows < 1 || frames < 1 || frames > 65535 || to.bpp < 1 || to.bpp > 4 || map_bytes > ((int64_t)1 << 32) || !fits)
        what = "the batch does not fit one launch";
    else if (also) what = also;
    else if (!maps_aligned || (!carry && to.floatmap && ((uintptr_t)to.out | (uintptr_t)to.frame_stride) % 4 != 0))
        what = "the float maps are not aligned";
    if (!what) return 0;
    *err = std::string(who) + ": " + what;
    return -1;
}

int launch_shutter_combine_clip(const ClipSamples &in, const ClipStore &to, int region_w, int rows, int render_w, float inv_k, int frames,
                                NativeWorkspace &ws, hipStream_t s, std::string *err) {
    const int64_t map_bytes = (int64_t)rows * render_w * 16;
    if (check_clip_launch("shutter combine", to, in.carry_out != nullptr, region_w, rows, frames, map_bytes, render_w >= region_w && in.count >= 1,
                          nullptr, clip_maps_aligned(in), err) != 0)
        return -1;
    ShutterArgs a;
    a.samples = (const unsigned char *)in.samples;
    a.carry_in = (unsigned char *)in.carry_in;
    a.carry_out = (unsigned char *)in.carry_out;
    a.out = (unsigned char *)to.out;
    a.sample_stride = in.sample_stride;
    a.frame_samples_stride = in.frame_samples_stride;
    a.carry_frame_stride = map_bytes;
    a.frame_stride = to.frame_stride;
    a.row_stride = to.row_stride;
    a.count = in.count;
    a.region_w = (unsigned)region_w;
    a.render_w = (unsigned)render_w;
    a.items = (unsigned)region_w * (unsigned)rows;
    a.inv_k = inv_k;
    const dim3 grid((a.items + 255u) / 256u, (unsigned)frames);
    ws.timed_launch("shutter_combine_clip", s, [&] {
        with_store_mode(clip_store_mode(to, in.carry_out != nullptr), [&](auto mode) { k_shutter_combine_clip<mode()><<<grid, 256, 0, s>>>(a); });
    });
    if (hipGetLastError() != hipSuccess) { *err = "shutter combine: kernel launch failed"; return -1; }
    return 0;
}

// ---- the contrast mask of an adaptively anti-aliased clip (mmhip_render_clip_adaptive states the rule) ----
// Frame blockIdx.y of a batch per grid row, one tile of AA_TILE_W x AA_TILE_H pixels of the rendered rectangle per
// workgroup, one pixel per lane.  A lane loads its own texel of the base map (kept as loaded for the store, clamped into
// LDS), the first 84 lanes the tile's one-pixel halo; texels outside the rectangle are neither loaded nor compared.  A
// pixel that is not refined is stored as the shutter combine stores a single sample; a refined one is counted -- one
// atomicAdd per workgroup -- and, with LIST, appended to the frame's list as col | rl << 16 at the place its rank among
// the workgroup's refined lanes (ballot, popcount) gives it in the range that atomicAdd reserved.
struct AaArgs {
    const unsigned char *base;
    unsigned char *out;
    unsigned *counts, *list;
    long long base_frame_stride, frame_stride, list_stride;
    int row_stride;
    unsigned region_w, rows, render_w, tiles_x;
    float threshold, inv_k;
};

constexpr int AA_TILE_W = 32, AA_TILE_H = 8, AA_HALO = 2 * (AA_TILE_W + 2) + 2 * AA_TILE_H;
static_assert(AA_TILE_W * AA_TILE_H == 256 && AA_HALO <= 256, "one lane per pixel of the tile, the halo by the first lanes");

__device__ __forceinline__ float aa_clamp(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
__device__ __forceinline__ sh_f32x4 aa_clamp4(sh_f32x4 f) {
    sh_f32x4 r;
    r.x = aa_clamp(f.x);
    r.y = aa_clamp(f.y);
    r.z = aa_clamp(f.z);
    r.w = aa_clamp(f.w);
    return r;
}
// one f32 subtraction per channel; a NaN contrast refines
__device__ __forceinline__ bool aa_contrast(sh_f32x4 p, sh_f32x4 q, float threshold) {
    return !(fabsf(p.x - q.x) <= threshold) || !(fabsf(p.y - q.y) <= threshold) || !(fabsf(p.z - q.z) <= threshold) ||
           !(fabsf(p.w - q.w) <= threshold);
}

template <int MODE, bool LIST>
__global__ void __launch_bounds__(256) k_aa_contrast_clip(const AaArgs a) {
    __shared__ sh_f32x4 tile[AA_TILE_H + 2][AA_TILE_W + 2];
    __shared__ unsigned wave_n[4], wg_base;
    const unsigned ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = (int)tx * AA_TILE_W, y0 = (int)ty * AA_TILE_H, w = (int)a.region_w, h = (int)a.rows;
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ F = a.base + fi * a.base_frame_stride;
    const int lx = threadIdx.x % AA_TILE_W, ly = threadIdx.x / AA_TILE_W;
    const int col = x0 + lx, rl = y0 + ly;
    const bool inside = col < w && rl < h;
    const unsigned off = ((unsigned)rl * a.render_w + (unsigned)col) * 16u;      // below 2^32: the launcher refuses larger maps
    sh_f32x4 raw = {0.0f, 0.0f, 0.0f, 0.0f};
    if (inside) {
        raw = *(const sh_f32x4 *)(F + off);
        tile[ly + 1][lx + 1] = aa_clamp4(raw);
    }
    if (threadIdx.x < AA_HALO) {
        const int k = threadIdx.x;
        int hx, hy;
        if (k < AA_TILE_W + 2) { hx = k - 1; hy = -1; }
        else if (k < 2 * (AA_TILE_W + 2)) { hx = k - (AA_TILE_W + 2) - 1; hy = AA_TILE_H; }
        else if (k < 2 * (AA_TILE_W + 2) + AA_TILE_H) { hx = -1; hy = k - 2 * (AA_TILE_W + 2); }
        else { hx = AA_TILE_W; hy = k - 2 * (AA_TILE_W + 2) - AA_TILE_H; }
        const int gx = x0 + hx, gy = y0 + hy;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h)
            tile[hy + 1][hx + 1] = aa_clamp4(*(const sh_f32x4 *)(F + ((unsigned)gy * a.render_w + (unsigned)gx) * 16u));
    }
    __syncthreads();
    bool refine = false;
    if (inside) {
        refine = a.threshold < 0.0f;
        const sh_f32x4 p = tile[ly + 1][lx + 1];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dx == 0 && dy == 0) continue;
                const int qx = col + dx, qy = rl + dy;
                if (qx >= 0 && qx < w && qy >= 0 && qy < h && aa_contrast(p, tile[ly + 1 + dy][lx + 1 + dx], a.threshold)) refine = true;
            }
    }
    if (inside && !refine) clip_store_mean<MODE, false>(raw, a.inv_k, a.out, fi, a.frame_stride, [off] { return off; }, (long long)rl, a.row_stride, (unsigned)col);
    const unsigned long long ballot = __ballot(refine);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = (unsigned)__popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        wg_base = total ? atomicAdd(a.counts + fi, total) : 0u;
    }
    if (LIST) {
        __syncthreads();
        if (refine) {
            unsigned at = wg_base + (unsigned)__popcll(ballot & ((1ull << lane) - 1ull));
            for (unsigned k = 0; k < wave; ++k) at += wave_n[k];
            a.list[fi * a.list_stride + at] = (unsigned)col | ((unsigned)rl << 16);
        }
    }
}

int launch_aa_contrast_clip(const void *base, int64_t base_frame_stride, const ClipStore &to, const ClipRefined &refined, int region_w, int rows,
                            int render_w, float threshold, int frames, NativeWorkspace &ws, hipStream_t s, std::string *err) {
    const bool listed = refined.list != nullptr;
    if (check_clip_launch("aa contrast", to, false, region_w, rows, frames, (int64_t)rows * render_w * 16,
                          render_w >= region_w &&
                              !(listed && (region_w > 65535 || rows > 65535 || refined.list_stride < (int64_t)region_w * rows)),
                          nullptr, ((uintptr_t)base | (uintptr_t)base_frame_stride) % 16 == 0, err) != 0)
        return -1;
    AaArgs a;
    a.base = (const unsigned char *)base;
    a.out = (unsigned char *)to.out;
    a.counts = refined.counts;
    a.list = refined.list;
    a.base_frame_stride = base_frame_stride;
    a.frame_stride = to.frame_stride;
    a.list_stride = refined.list_stride;
    a.row_stride = to.row_stride;
    a.region_w = (unsigned)region_w;
    a.rows = (unsigned)rows;
    a.render_w = (unsigned)render_w;
    a.tiles_x = ((unsigned)region_w + AA_TILE_W - 1) / AA_TILE_W;
    a.threshold = threshold;
    a.inv_k = mm_shutter_inv_k(1);
    const dim3 grid(a.tiles_x * (((unsigned)rows + AA_TILE_H - 1) / AA_TILE_H), (unsigned)frames);
    ws.timed_launch("aa_contrast_clip", s, [&] {
        with_store_mode(clip_store_mode(to, false), [&](auto mode) {
            if constexpr (mode() != CLIP_CARRY) {      // the mask has no carry pass
                if (listed) k_aa_contrast_clip<mode(), true><<<grid, 256, 0, s>>>(a);
                else k_aa_contrast_clip<mode(), false><<<grid, 256, 0, s>>>(a);
            }
        });
    });
    if (hipGetLastError() != hipSuccess) { *err = "aa contrast: kernel launch failed"; return -1; }
    return 0;
}

// ---- the reconstruction filter of an anti-aliased clip (mmhip_render_clip_filtered states the arithmetic) ----
// Frame blockIdx.y of a batch per grid row, one tile of FC_TILE_W x FC_TILE_H output pixels per workgroup, one pixel per
// lane.  Per time step of the pass, stage one sums along the row: h_b of the tile's columns over the tile's rows and D
// halo rows either side, for every grid row b, into LDS as float4 [halo row][b][column] -- a wave reads 512 adjacent
// bytes per tap from a sub-sample map.  After a barrier stage two sums down the column out of LDS and adds the step to
// the lane's accumulator.  The taps come from the block of the pixel's edge class (mm_clip_filter_compact: the taps that
// are read, in tap order, with their places); a workgroup whose columns (rows) are all interior reads it through a
// wave-uniform pointer, so those loads are scalar.  A tap of weight 0 -- one outside the frame among them -- is in no
// block and so is never read; the offset it would have may lie outside the map.  Offsets inside a map are 32-bit, from
// wave-uniform bases that advance by sample_stride.  The sub-samples are loaded as ordinary cached loads: a texel is
// read by several taps of neighbouring lanes and by the tile below, and with non-temporal loads every one of those
// reads went out to memory again (measured: 2.8 against 1.9 times the plain combine at D = 1); the
// stores of the output are non-temporal.  LDS: (FC_TILE_H + 2 D) * sy * FC_TILE_W * 16 bytes, 64 KiB at D = 4 and
// sy = 8, two workgroups to a CU.
struct FilterArgs {
    const unsigned char *samples;
    unsigned char *carry_in, *carry_out, *out;
    const unsigned *wx, *wy;                              // (D + 1)^2 tap blocks per axis, by edge class (mm_clip_filter_compact)
    long long sample_stride, frame_samples_stride, carry_frame_stride, frame_stride;
    int row_stride, count, sx, sy, reach;                 // count: the time steps of the pass, sx * sy maps each
    int region_x, first_row;                              // frame column and row of output pixel (0, 0)
    int hx0, hy0, hy1;                                    // the haloed rectangle the maps hold: its first column, its rows
    unsigned region_w, rows, render_w, render_h, tiles_x;
    float inv_k;
};

constexpr int FC_TILE_W = 32, FC_TILE_H = 8;
static_assert(FC_TILE_W * FC_TILE_H == 256, "one lane per pixel of the tile");
static_assert((FC_TILE_H + 2 * MM_CLIP_FILTER_MAX_REACH) * MM_SAMPLE_GRID_MAX * FC_TILE_W * 16 <= 65536, "the worst case fits LDS twice per CU");

__device__ __forceinline__ sh_f32x4 fc_first(float w, sh_f32x4 f) {
    sh_f32x4 r;
    r.x = mm_clip_filter_first(w, f.x);
    r.y = mm_clip_filter_first(w, f.y);
    r.z = mm_clip_filter_first(w, f.z);
    r.w = mm_clip_filter_first(w, f.w);
    return r;
}
__device__ __forceinline__ sh_f32x4 fc_next(sh_f32x4 acc, float w, sh_f32x4 f) {
    sh_f32x4 r;
    r.x = mm_clip_filter_next(acc.x, w, f.x);
    r.y = mm_clip_filter_next(acc.y, w, f.y);
    r.z = mm_clip_filter_next(acc.z, w, f.z);
    r.w = mm_clip_filter_next(acc.w, w, f.w);
    return r;
}

// h_b of one texel: the taps of block `blk` (mm_clip_filter_compact: only those that are read, in tap order) over the
// maps of grid row b, which begin at G0 and lie sample_stride apart; off0 is the byte offset of the texel at dx = -D
// (formed modulo 2^32: only existing taps are dereferenced).  Four loads ahead of their four sums.
__device__ __forceinline__ sh_f32x4 fc_row_sum(const unsigned char *__restrict__ G0, long long sample_stride, unsigned off0,
                                               const unsigned *__restrict__ blk, int taps) {
    const int count = (int)blk[0];
    const unsigned *__restrict__ wt = blk + 1, *__restrict__ place = blk + 1 + taps;
    auto texel = [&](int t) {
        const unsigned p = place[t];
        return *(const sh_f32x4 *)(G0 + (long long)(p & 255u) * sample_stride + (off0 + (p >> 8) * 16u));
    };
    auto weight = [&](int t) { return __builtin_bit_cast(float, wt[t]); };
    if (count < 1) return sh_f32x4{0.0f, 0.0f, 0.0f, 0.0f};      // (no class that occurs is empty)
    sh_f32x4 acc = fc_first(weight(0), texel(0));
    int t = 1;
    for (; t + 4 <= count; t += 4) {
        const sh_f32x4 f0 = texel(t), f1 = texel(t + 1), f2 = texel(t + 2), f3 = texel(t + 3);
        acc = fc_next(fc_next(fc_next(fc_next(acc, weight(t), f0), weight(t + 1), f1), weight(t + 2), f2), weight(t + 3), f3);
    }
    for (; t < count; ++t) acc = fc_next(acc, weight(t), texel(t));
    return acc;
}

// s_j of one pixel: the taps (dy, b) of block `blk` over the column of h in LDS that begins at h0 (halo row 0 of the
// lane's window, grid row 0).
__device__ __forceinline__ sh_f32x4 fc_column_sum(const sh_f32x4 *h0, const unsigned *__restrict__ blk, int taps, int sy) {
    const int count = (int)blk[0];
    const unsigned *__restrict__ wt = blk + 1, *__restrict__ place = blk + 1 + taps;
    auto texel = [&](int t) {
        const unsigned p = place[t];
        return h0[((p >> 8) * (unsigned)sy + (p & 255u)) * FC_TILE_W];
    };
    auto weight = [&](int t) { return __builtin_bit_cast(float, wt[t]); };
    if (count < 1) return sh_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    sh_f32x4 acc = fc_first(weight(0), texel(0));
    int t = 1;
    for (; t + 4 <= count; t += 4) {
        const sh_f32x4 f0 = texel(t), f1 = texel(t + 1), f2 = texel(t + 2), f3 = texel(t + 3);
        acc = fc_next(fc_next(fc_next(fc_next(acc, weight(t), f0), weight(t + 1), f1), weight(t + 2), f2), weight(t + 3), f3);
    }
    for (; t < count; ++t) acc = fc_next(acc, weight(t), texel(t));
    return acc;
}

template <int MODE>
__global__ void __launch_bounds__(256) k_filter_combine_clip(const FilterArgs a) {
    extern __shared__ sh_f32x4 fc_h[];      // [FC_TILE_H + 2 D][sy][FC_TILE_W]
    const unsigned ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int lx = threadIdx.x % FC_TILE_W, ly = threadIdx.x / FC_TILE_W;
    const int D = a.reach, sx = a.sx, sy = a.sy;
    const int col0 = (int)tx * FC_TILE_W, row0 = (int)ty * FC_TILE_H;
    const int col = col0 + lx, row = row0 + ly;
    const bool col_in = col < (int)a.region_w, inside = col_in && row < (int)a.rows;
    const int x = a.region_x + (col_in ? col : 0), y = a.first_row + (inside ? row : 0);      // the lane's pixel in the frame
    // the tile's last column and row in the frame: are all of its pixels interior along an axis?
    const int col_end = col0 + FC_TILE_W < (int)a.region_w ? col0 + FC_TILE_W : (int)a.region_w;
    const int row_end = row0 + FC_TILE_H < (int)a.rows ? row0 + FC_TILE_H : (int)a.rows;
    const int x_last = a.region_x + col_end - 1, y_last = a.first_row + row_end - 1;
    const bool uniform_x = a.region_x + col0 >= D && x_last + D < (int)a.render_w;
    const bool uniform_y = a.first_row + row0 >= D && y_last + D < (int)a.render_h;
    const int interior = D * (D + 1) + D, taps_x = mm_clip_filter_tap_count(D, sx), taps_y = mm_clip_filter_tap_count(D, sy);
    const int block_x = mm_clip_filter_block_words(taps_x), block_y = mm_clip_filter_block_words(taps_y);
    const unsigned *__restrict__ wx_lane = a.wx + mm_clip_filter_class(x, (int)a.render_w, D) * block_x;
    const unsigned *__restrict__ wy_lane = a.wy + mm_clip_filter_class(y, (int)a.render_h, D) * block_y;
    const unsigned *__restrict__ wx_all = a.wx + interior * block_x;
    const unsigned *__restrict__ wy_all = a.wy + interior * block_y;
    const size_t fi = blockIdx.y;
    const unsigned char *__restrict__ S = a.samples + fi * a.frame_samples_stride;
    const long long step_stride = (long long)sx * sy * a.sample_stride, grid_row_stride = (long long)sx * a.sample_stride;
    const int halo_rows = FC_TILE_H + 2 * D;
    const unsigned off_carry = ((unsigned)row * a.region_w + (unsigned)col) * 16u;      // the carry maps are packed
    sh_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (a.carry_in && inside) acc = *(const sh_f32x4 *)(a.carry_in + fi * a.carry_frame_stride + off_carry);
    for (int j = 0; j < a.count; ++j, S += step_stride) {
        for (int it = ly; it < halo_rows * sy; it += FC_TILE_H) {
            const int rr = it / sy, b = it - rr * sy;
            const int yy = a.first_row + row0 - D + rr;      // the frame row of halo row rr
            if (col_in && yy >= a.hy0 && yy < a.hy1) {
                const unsigned off0 = ((unsigned)(yy - a.hy0) * a.render_w + (unsigned)(x - D - a.hx0)) * 16u;
                const unsigned char *__restrict__ G0 = S + b * grid_row_stride;
                fc_h[it * FC_TILE_W + lx] = uniform_x ? fc_row_sum(G0, a.sample_stride, off0, wx_all, taps_x)
                                                      : fc_row_sum(G0, a.sample_stride, off0, wx_lane, taps_x);
            }
        }
        __syncthreads();
        if (inside) {
            const sh_f32x4 *h0 = fc_h + (ly * sy) * FC_TILE_W + lx;
            const sh_f32x4 sj = uniform_y ? fc_column_sum(h0, wy_all, taps_y, sy) : fc_column_sum(h0, wy_lane, taps_y, sy);
            acc = (j == 0 && !a.carry_in) ? sj : shutter_add(acc, sj);
        }
        __syncthreads();
    }
    if (!inside) return;
    if constexpr (MODE == CLIP_CARRY) *(sh_f32x4 *)(a.carry_out + fi * a.carry_frame_stride + off_carry) = acc;
    else
        clip_store_mean<MODE, true>(acc, a.inv_k, a.out, fi, a.frame_stride, [row, col, w = a.render_w] { return ((unsigned)row * w + (unsigned)col) * 16u; },
                                    (long long)row, a.row_stride, (unsigned)col);
}

int launch_filter_combine_clip(const ClipSamples &in, const ClipFilterTaps &taps, const ClipStore &to, const ClipRect &r, float inv_k, int frames,
                               NativeWorkspace &ws, hipStream_t s, std::string *err) {
    const int sx = taps.sx, sy = taps.sy, reach = taps.reach;
    const bool fits = in.count >= 1 && sx >= 1 && sx <= MM_SAMPLE_GRID_MAX && sy >= 1 && sy <= MM_SAMPLE_GRID_MAX && reach >= 0 &&
                      reach <= MM_CLIP_FILTER_MAX_REACH && taps.wx && taps.wy && r.render_w >= 1 && r.render_h >= 1;
    // the output rectangle inside the frame, and every neighbour of it that is inside the frame inside the maps
    const bool holds = !fits ||
                       !(r.region_x < 0 || r.first_row < 0 || (int64_t)r.region_x + r.region_w > r.render_w ||
                         (int64_t)r.first_row + r.rows > r.render_h || r.halo_x < 0 || r.halo_y < 0 || r.halo_w < 1 || r.halo_rows < 1 ||
                         (int64_t)r.halo_x + r.halo_w > r.render_w || (int64_t)r.halo_y + r.halo_rows > r.render_h ||
                         r.halo_x > std::max(0, r.region_x - reach) || r.halo_x + r.halo_w < std::min(r.render_w, r.region_x + r.region_w + reach) ||
                         r.halo_y > std::max(0, r.first_row - reach) || r.halo_y + r.halo_rows < std::min(r.render_h, r.first_row + r.rows + reach));
    if (check_clip_launch("filter combine", to, in.carry_out != nullptr, r.region_w, r.rows, frames, (int64_t)r.halo_rows * r.render_w * 16, fits,
                          holds ? nullptr : "the maps do not hold the output rectangle and its neighbours",
                          clip_maps_aligned(in) && ((uintptr_t)taps.wx | (uintptr_t)taps.wy) % 4 == 0, err) != 0)
        return -1;
    FilterArgs a;
    a.samples = (const unsigned char *)in.samples;
    a.carry_in = (unsigned char *)in.carry_in;
    a.carry_out = (unsigned char *)in.carry_out;
    a.out = (unsigned char *)to.out;
    a.wx = taps.wx;
    a.wy = taps.wy;
    a.sample_stride = in.sample_stride;
    a.frame_samples_stride = in.frame_samples_stride;
    a.carry_frame_stride = (int64_t)r.rows * r.region_w * 16;
    a.frame_stride = to.frame_stride;
    a.row_stride = to.row_stride;
    a.count = in.count;
    a.sx = sx;
    a.sy = sy;
    a.reach = reach;
    a.region_x = r.region_x;
    a.first_row = r.first_row;
    a.hx0 = r.halo_x;
    a.hy0 = r.halo_y;
    a.hy1 = r.halo_y + r.halo_rows;
    a.region_w = (unsigned)r.region_w;
    a.rows = (unsigned)r.rows;
    a.render_w = (unsigned)r.render_w;
    a.render_h = (unsigned)r.render_h;
    a.tiles_x = ((unsigned)r.region_w + FC_TILE_W - 1) / FC_TILE_W;
    a.inv_k = inv_k;
    const dim3 grid(a.tiles_x * (((unsigned)r.rows + FC_TILE_H - 1) / FC_TILE_H), (unsigned)frames);
    const size_t lds = (size_t)(FC_TILE_H + 2 * reach) * sy * FC_TILE_W * 16;
    ws.timed_launch("filter_combine_clip", s, [&] {
        with_store_mode(clip_store_mode(to, in.carry_out != nullptr), [&](auto mode) { k_filter_combine_clip<mode()><<<grid, 256, lds, s>>>(a); });
    });
    if (hipGetLastError() != hipSuccess) { *err = "filter combine: kernel launch failed"; return -1; }
    return 0;
}

}  // namespace mm
