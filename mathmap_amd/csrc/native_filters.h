// Native filters (the reference's native-filters/*.c) as hand-written HIP kernels.
// Called by the runtime between the prologue and the pixel kernel; inputs and
// outputs stay in HBM.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "mm_host_abi.h"

namespace mm {

// What render_image's pixel fetch reads from the invocation (builtins.c:120-159: get_orig_val_pixel
// is hard-wired there -- nearest, never bilinear -- but it still honours the invocation's
// supersampling flag, edge behaviours and edge colours).
struct NativeEnv {
    int supersampling = 0;
    int edge_x = 0, edge_y = 0;                 // 0 colour, 1 wrap, 2 reflect, 3 rotate
    uint32_t edge_color_x = 0, edge_color_y = 0;
};

// Scratch buffers reused across calls (sized for the largest map seen).
struct NativeWorkspace {
    NativeEnv env;                              // set by the runtime before every run_native_filter
    bool gauss_tolerance = false;               // so is this: the filter's gauss_mode is MMHIP_GAUSS_TOLERANCE (include/mmhip.h)
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    bool keep_tolerance_map = false;            // test hook (abi_selftest.cpp): the tolerance chain writes the map too
    void *reserve(size_t bytes);
    void release();
    // per-kernel timing of a native filter's own launches (mmhip_enable_timing): one HIP event pair per
    // launch on the launch stream, read back by mmhip_drain_native_kernel_ms
    struct Timed { const char *name; hipEvent_t a, b; };
    bool timing = false;
    std::vector<Timed> timed;                   // launches since the last drain, in launch order
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timed_free;
    // brackets `launch()` with an event pair when timing is on
    template <class F> void timed_launch(const char *name, hipStream_t s, F &&launch) {
        if (!timing || timed.size() >= 4096) { launch(); return; }
        Timed t{name, nullptr, nullptr};
        if (!timed_free.empty()) { t.a = timed_free.back().first; t.b = timed_free.back().second; timed_free.pop_back(); }
        else if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) { launch(); return; }
        (void)hipEventRecord(t.a, s);
        launch();
        (void)hipEventRecord(t.b, s);
        timed.push_back(t);
    }
    // cached hipFFT plans of the FFT native filters (native_fft.hip)
    void *fft_fwd = nullptr, *fft_inv = nullptr;
    int fft_w = 0, fft_h = 0, fft_batch = 0;
    bool fft_valid = false;
};

// Runs native filter `func` with the arguments recorded by the prologue kernel.
// `out_map` is a float[h][w][4] device buffer.  Returns 0 on success.
// `row_lo, row_hi`: the rows of the map the caller is going to read.  Filters whose output
// rows depend on a bounded neighbourhood of input rows (gaussian_blur: a halo of ceil(22.7 sigma)
// rows, below which the recurrences' start-up error is under 1e-17 of the value) may fill only
// those rows plus their halo; [0, render_h) asks for the whole map.
// Optional direct output of a native filter (new_template.c.in:279-293 applied to the filter's own
// result): when the calling filter's pixel is just this result sampled at the pixel centre, the
// filter's last kernel also writes the RGBA8 pixels of rows [first_row, first_row + num_rows) x
// columns [region_x, region_x + region_w) and the pixel kernel is not launched.  `written` reports
// whether the path taken supports it (the recursive Gaussian does).
struct NativeDirectOut {
    void *out = nullptr;          // first requested row, first requested column
    int row_stride = 0;           // bytes
    int first_row = 0, num_rows = 0, region_x = 0, region_w = 0;
    bool skip_map = false;        // in: the caller will not read the float map (it is not memoised): do not write it
    bool written = false;         // out; with skip_map the map's contents are then undefined
    bool tolerance = false;       // out: written by gaussian_blur's tolerance chain (gauss_mode)
};

int run_native_filter(const std::string &func, const HNativeRec &rec, const std::vector<HImageDesc> &images,
                      int render_w, int render_h, float *out_map, NativeWorkspace &ws, hipStream_t stream,
                      std::string *err, int *row_lo, int *row_hi,    // in: rows wanted, out: rows filled
                      NativeDirectOut *direct = nullptr);

// How gaussian_blur splits one pass of its recursive path: lines of `n` steps, `lines` of them, a deviation of `sigma`
// pixels; `tolerance`: the tolerance chain's plan instead of the exact chain's (which reads MMHIP_GAUSS_SEGMENTS per call).
// out = {segment length, warm-up halo, number of segments}.  Read-only, for tests (abi_selftest.cpp).
void gaussian_blur_line_plan(int n, int lines, float sigma, int tolerance, int out[3]);

// ---- gaussian_blur over the frames of a clip (mmhip_render_clip) ----
// One computation of a batch: a gaussian_blur call whose image argument is either a bound drawable of the render size
// under the identity mapping or an earlier computation's float map, and whose deviations are at least half a pixel
// (the recursive chain, exact).  gaussian_blur_batchable says whether a recorded call is one, by the decisions of the
// single-frame chain itself; `ckpt_bytes` / `map_bytes` (either may be null) receive what one job needs of each.
bool gaussian_blur_batchable(const HNativeRec &rec, const HImageDesc *images, int num_images, int render_w, int render_h,
                             const NativeEnv &env, size_t *ckpt_bytes, size_t *map_bytes);
void gaussian_blur_batch_job_bytes(int render_w, int render_h, size_t *ckpt_bytes, size_t *map_bytes);
struct GaussClipJob {
    HNativeRec rec;                 // the call as the prologue recorded it
    const HImageDesc *images;       // the image table of the job's frame (rec's image argument indexes it)
    int num_images;
    double *ckpt;                   // ckpt_bytes of its own
    float *mapT;                    // map_bytes of its own: the first pass's transposed result
    float *out_map;                 // map_bytes: the result (unused where the launch writes no map)
    unsigned char *pack_out;        // the first byte of the job's band of RGBA8 pixels (direct output), or null
};
// What all jobs of one gaussian_blur_batch share.  `direct`: rows, columns and row stride of the bands the second pass
// packs (its `out` is not read: every job has its own pack_out); null = no job packs.
struct GaussClipLaunch {
    int render_w = 0, render_h = 0;
    const NativeDirectOut *direct = nullptr;
    bool write_map = true;          // false: only the packed pixels leave the second pass
};
// Device-table bytes gaussian_blur_batch needs for `jobs` jobs.
size_t gaussian_blur_batch_table_bytes(size_t jobs);
// Fills `host_table` (gaussian_blur_batch_table_bytes) for the jobs; `device_table` is where the caller is going to copy
// it before gaussian_blur_batch_launch runs.  Returns the groups to launch (jobs of one source type each) in `groups`.
struct GaussClipGroup { bool drawable; unsigned jobs; const void *vertical, *horizontal; unsigned pitch; };
int gaussian_blur_batch_tables(const std::vector<GaussClipJob> &jobs, const GaussClipLaunch &launch, const NativeEnv &env,
                               char *host_table, const char *device_table, std::vector<GaussClipGroup> *groups, std::string *err);
// Four launches per group (iir_causal_vertical_clip, iir_anticausal_vertical_clip, iir_causal_horizontal_clip,
// iir_anticausal_horizontal_clip), timed through ws.timed_launch.
int gaussian_blur_batch_launch(const std::vector<GaussClipGroup> &groups, const GaussClipLaunch &launch, NativeWorkspace &ws,
                               hipStream_t s, std::string *err);

// native_fft.hip: convolve / half_convolve / visualize_fft (native-filters/convolve.c)
int fft_native_filter(const std::string &func, const HNativeRec &rec, const std::vector<HImageDesc> &images, int render_w,
                      int render_h, float *out_map, NativeWorkspace &ws, hipStream_t stream, std::string *err);
int native_input_map(const char *who, const HImage &img, const std::vector<HImageDesc> &images, const NativeEnv &env, int w,
                     int h, float *dst, const float **map, hipStream_t s, std::string *err);
void fft_release_plans(NativeWorkspace &ws);
// render_image, drawable branch (builtins.c:303-343): `dst` = float[h][w][4]
void launch_render_drawable(const HImageDesc &in, const HImage &img, const NativeEnv &env, float *dst, int w, int h, hipStream_t s);

void launch_supersample_combine(const unsigned char *longs, const unsigned char *shorts, unsigned char *out, int w, int h,
                                int bpp, int out_stride, hipStream_t s);
// The combine over `frames` supersampled frames of a clip in one launch (k_supersample_combine_clip): frame i's long slice
// at longs + i * h * long_pitch with rows supersample_clip_long_pitch(w, bpp) bytes apart, its short slice at shorts +
// i * h * w * bpp (packed), its output at out + i * frame_stride.  A work-item combines SS_CLIP_PIXELS adjacent pixels
// over SS_CLIP_ROWS rows; supersample_clip_items: the work-items of one frame (the launch takes fewer than 2^31).
// Timed through ws.timed_launch as supersample_combine_clip.
constexpr int SS_CLIP_ROWS = 8, SS_CLIP_PIXELS = 4;
size_t supersample_clip_long_pitch(int w, int bpp);
int64_t supersample_clip_items(int w, int h);
int launch_supersample_combine_clip(const unsigned char *longs, const unsigned char *shorts, unsigned char *out, int w, int h,
                                    int bpp, int row_stride, int64_t frame_stride, int frames, NativeWorkspace &ws, hipStream_t s,
                                    std::string *err);
// One pass of the temporal combine of a motion-blurred clip (k_shutter_combine_clip; mmhip_render_clip_shutter states the
// arithmetic, mm_shutter_combine.h holds it) over `frames` frames in one launch.  Sub-sample j of the pass (0 <= j <
// count) of frame i is a float map of `rows` rows of render_w float4 at samples + i * frame_samples_stride + j *
// sample_stride, the region's region_w columns at the start of each row.  The sum starts from the first sub-sample
// where carry_in is null, else from frame i's carry map (rows * render_w float4, the frames packed).  With carry_out
// the pass writes the running sum there and nothing else (carry_out may be carry_in); without, it scales by inv_k and
// stores frame i at out + i * frame_stride: float4 rows 16 * render_w bytes apart with `floatmap`, else the pixel
// store's bytes at output_bpp `bpp`, rows row_stride apart (32-bit stores where bpp is 4 and out, row_stride and
// frame_stride are multiples of 4).  Refused: maps beyond 2^32 bytes (offsets inside a frame are 32-bit), more than
// 65 535 frames, float maps that are not 16-byte aligned.  Timed through ws.timed_launch as shutter_combine_clip.
int launch_shutter_combine_clip(const void *samples, int64_t sample_stride, int64_t frame_samples_stride, int count, const void *carry_in,
                                void *carry_out, void *out, int region_w, int rows, int render_w, int row_stride, int64_t frame_stride,
                                int bpp, int floatmap, float inv_k, int frames, NativeWorkspace &ws, hipStream_t s, std::string *err);
// The contrast mask of an adaptively anti-aliased clip (k_aa_contrast_clip; mmhip_render_clip_adaptive states the rule)
// over `frames` frames in one launch.  Frame i's base map is `rows` rows of render_w float4 at base + i *
// base_frame_stride, the region's region_w columns at the start of each row.  A pixel that is not refined is stored at
// out + i * frame_stride as the shutter combine stores a single sample (the same store modes); a refined one is left
// alone, counted in counts[i] (which the caller has zeroed) and, where `list` is not null, appended to frame i's list at
// list + i * list_stride as col | rl << 16, in no particular order.  Refused: what the shutter combine refuses, and with
// a list a region beyond 65 535 columns or rows.  Timed through ws.timed_launch as aa_contrast_clip.
int launch_aa_contrast_clip(const void *base, int64_t base_frame_stride, void *out, unsigned *counts, unsigned *list, int64_t list_stride,
                            int region_w, int rows, int render_w, int row_stride, int64_t frame_stride, int bpp, int floatmap,
                            float threshold, int frames, NativeWorkspace &ws, hipStream_t s, std::string *err);
// One pass of the reconstruction filter of an anti-aliased clip (k_filter_combine_clip; mmhip_render_clip_filtered states
// the arithmetic, mm_clip_filter.h holds it) over `frames` frames in one launch.  The maps hold the haloed rectangle:
// columns [halo_x, halo_x + halo_w) by rows [halo_y, halo_y + halo_rows) of the render_w x render_h frame, as halo_rows
// rows of render_w float4 with the rectangle's columns at the start of each row.  Grid point g = b * sx + a of time step
// j of the pass (0 <= j < count) of frame i is at samples + i * frame_samples_stride + (j * sx * sy + g) * sample_stride.
// wx and wy, in device memory, are the (D + 1)^2 tap blocks of each axis by edge class (mm_clip_filter_axis_blocks), D = reach.
// The output is the rectangle of region_w columns from frame column region_x by `rows` rows from frame row first_row.
// The time sum starts from the first step where carry_in is null, else from frame i's carry map (rows * region_w
// float4, packed, the frames packed).  With carry_out the pass writes the running sum there and nothing else (carry_out
// may be carry_in); without, it scales by inv_k and stores frame i at out + i * frame_stride as
// launch_shutter_combine_clip does.  Refused: maps beyond 2^32 bytes, more than 65 535 frames, maps that do not hold
// every neighbour of the output rectangle that lies inside the frame, float maps that are not 16-byte aligned.  Timed
// through ws.timed_launch as filter_combine_clip.
int launch_filter_combine_clip(const void *samples, int64_t sample_stride, int64_t frame_samples_stride, int count, int sx, int sy, int reach,
                               const unsigned *wx, const unsigned *wy, const void *carry_in, void *carry_out, void *out, int region_x,
                               int first_row, int region_w, int rows, int halo_x, int halo_y, int halo_w, int halo_rows, int render_w,
                               int render_h, int row_stride, int64_t frame_stride, int bpp, int floatmap, float inv_k, int frames,
                               NativeWorkspace &ws, hipStream_t s, std::string *err);
// RGBA8 frames of a clip to planar Y'CbCr 4:2:0 in one launch (k_rgba8_to_yuv420_clip, clip_yuv.hip; mmhip_clip_to_yuv420
// states the semantics and its parameters are these, mm_yuv.h holds the arithmetic).  The launcher takes the path of
// aligned wide accesses where the width is a multiple of 8, src and both source strides are multiples of 16 and dst and
// dst_frame_stride multiples of 8, else the path of byte accesses: the same bytes.  Refused, by name, in `err` (the
// check alone needs no GPU): a size below 1 x 1, no frame or more than 65 535, an unknown matrix or range, rows outside
// the frame, an odd first_row, an odd last_row that is not the height, a src_row_stride below one row, a
// dst_frame_stride below one frame, a Y plane or a source band beyond 4 GiB.  Timed through ws.timed_launch as yuv420_clip.
int check_rgba8_to_yuv420_clip(const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height, int first_row,
                               int last_row, int frames, int matrix, int range, const void *dst, int64_t dst_frame_stride, std::string *err);
int launch_rgba8_to_yuv420_clip(const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height, int first_row,
                                int last_row, int frames, int matrix, int range, void *dst, int64_t dst_frame_stride, NativeWorkspace &ws,
                                hipStream_t s, std::string *err);
// Planar Y'CbCr 4:2:0 frames of a clip to drawable words in one launch (k_yuv420_to_rgba_clip, clip_yuv_in.hip;
// mmhip_clip_from_yuv420 states the semantics and its parameters are these, mm_yuv.h holds the arithmetic).  The launcher
// takes the path of aligned wide accesses (*path = 0) where the width is a multiple of 8, src and src_frame_stride are
// multiples of 8 and dst and dst_frame_stride multiples of 16, else the path of byte accesses (*path = 1): the same
// words.  Refused, by name, in `err` (the check alone needs no GPU): a size below 1 x 1, no frame or more than 65 535, an
// unknown matrix, range or chroma mode, null pointers, a stride below one frame, a dst_frame_stride that is no multiple
// of 4, a destination frame beyond 4 GiB.  Timed through ws.timed_launch as yuv420_to_rgba_clip.
int check_yuv420_to_rgba_clip(const void *src, int64_t src_frame_stride, int width, int height, int frames, int matrix, int range, int chroma,
                              const void *dst, int64_t dst_frame_stride, std::string *err);
int launch_yuv420_to_rgba_clip(const void *src, int64_t src_frame_stride, int width, int height, int frames, int matrix, int range, int chroma,
                               void *dst, int64_t dst_frame_stride, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err);

}  // namespace mm
