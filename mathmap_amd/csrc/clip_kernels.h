// Launchers of the hand-written kernels that finish a clip or convert its frames: the combines, the contrast mask and the
// reconstruction filter (clip_combine.hip), Y'CbCr 4:2:0 out (clip_yuv.hip, 10-bit from float frames: clip_yuv10.hip) and in (clip_yuv_in.hip,
// 10-bit to float frames: clip_yuv10_in.hip): one job record, one check and one launcher per converter; what the four
// files share among themselves is in clip_yuv_common.h.
#pragma once
#include "native_filters.h"      // NativeWorkspace

namespace mm {

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

// ---- the shutter combine, the contrast mask and the filter combine: their argument records ----
// Where a batch's pixels go: frame i at out + i * frame_stride, as float4 rows 16 * render_w bytes apart with `floatmap`,
// else as the pixel store's bytes at output_bpp `bpp`, rows row_stride apart (32-bit stores where bpp is 4 and out,
// row_stride and frame_stride are multiples of 4).
struct ClipStore {
    void *out;
    int row_stride;
    int64_t frame_stride;
    int bpp, floatmap;
};
// The float maps one pass sums: map j of the pass (0 <= j < count) of frame i at samples + i * frame_samples_stride + j *
// sample_stride.  The sum starts from the first map where carry_in is null, else from frame i's carry map (the frames
// packed).  With carry_out the pass writes the running sum there and nothing else (carry_out may be carry_in).
struct ClipSamples {
    const void *samples;
    int64_t sample_stride, frame_samples_stride;
    int count;
    const void *carry_in;
    void *carry_out;
};
// The rectangles of the filter combine in a render_w x render_h frame: the output's region_w columns from frame column
// region_x by `rows` rows from frame row first_row, and the haloed one the maps hold, columns [halo_x, halo_x + halo_w) by
// rows [halo_y, halo_y + halo_rows).
struct ClipRect { int region_x, first_row, region_w, rows, halo_x, halo_y, halo_w, halo_rows, render_w, render_h; };
// The taps of the filter combine over an sx x sy grid: wx and wy, in device memory, are the (D + 1)^2 tap blocks of each
// axis by edge class (mm_clip_filter_axis_blocks), D = reach.
struct ClipFilterTaps { int sx, sy, reach; const unsigned *wx, *wy; };
// What the contrast mask reports: refined pixels counted in counts[i] (which the caller has zeroed) and, where `list` is
// not null, appended to frame i's list at list + i * list_stride as col | rl << 16, in no particular order.
struct ClipRefined { unsigned *counts, *list; int64_t list_stride; };

// One pass of the temporal combine of a motion-blurred clip (k_shutter_combine_clip; mmhip_render_clip_shutter states the
// arithmetic, mm_shutter_combine.h holds it) over `frames` frames in one launch.  A sub-sample is a float map of `rows`
// rows of render_w float4, the region's region_w columns at the start of each row; a carry map is one too.  Without
// carry_out the pass scales by inv_k and stores to `to`.  Refused: maps beyond 2^32 bytes (offsets inside a frame are
// 32-bit), more than 65 535 frames, float maps that are not 16-byte aligned.  Timed through ws.timed_launch as
// shutter_combine_clip.
int launch_shutter_combine_clip(const ClipSamples &in, const ClipStore &to, int region_w, int rows, int render_w, float inv_k, int frames,
                                NativeWorkspace &ws, hipStream_t s, std::string *err);
// The contrast mask of an adaptively anti-aliased clip (k_aa_contrast_clip; mmhip_render_clip_adaptive states the rule)
// over `frames` frames in one launch.  Frame i's base map is `rows` rows of render_w float4 at base + i *
// base_frame_stride, the region's region_w columns at the start of each row.  A pixel that is not refined is stored to
// `to` as the shutter combine stores a single sample (the same store modes); a refined one is left alone and reported
// in `refined`.  Refused: what the shutter combine refuses, and with a list a region beyond 65 535 columns or rows.
// Timed through ws.timed_launch as aa_contrast_clip.
int launch_aa_contrast_clip(const void *base, int64_t base_frame_stride, const ClipStore &to, const ClipRefined &refined, int region_w, int rows,
                            int render_w, float threshold, int frames, NativeWorkspace &ws, hipStream_t s, std::string *err);
// One pass of the reconstruction filter of an anti-aliased clip (k_filter_combine_clip; mmhip_render_clip_filtered states
// the arithmetic, mm_clip_filter.h holds it) over `frames` frames in one launch.  A map holds the haloed rectangle as
// halo_rows rows of render_w float4 with the rectangle's columns at the start of each row.  in.count is the time steps of
// the pass, of sx * sy maps each: grid point g = b * sx + a of step j is map j * sx * sy + g.  A carry map is rows *
// region_w float4, packed.  Without carry_out the pass scales by inv_k and stores to `to` as launch_shutter_combine_clip
// does.  Refused: maps beyond 2^32 bytes, more than 65 535 frames, maps that do not hold every neighbour of the output
// rectangle that lies inside the frame, float maps that are not 16-byte aligned.  Timed through ws.timed_launch as
// filter_combine_clip.
int launch_filter_combine_clip(const ClipSamples &in, const ClipFilterTaps &taps, const ClipStore &to, const ClipRect &r, float inv_k, int frames,
                               NativeWorkspace &ws, hipStream_t s, std::string *err);

// ---- the Y'CbCr 4:2:0 converters: their job records ----
// `name` is the entry point the refusals speak for (mmhip_<name>); matrix, range, chroma and siting are mm_yuv.h's.  Centre
// siting launches the SITING = MM_YUV_SITING_CENTER instantiations, left siting the SITING = MM_YUV_SITING_LEFT ones.
// Frames out: frame i's source rows [first_row, last_row) from src + i * src_frame_stride (src is the band's first row),
// rows src_row_stride bytes apart; its planes at dst + i * dst_frame_stride.
struct YuvOutJob {
    const char *name;
    const void *src;
    int64_t src_row_stride, src_frame_stride;
    int width, height, first_row, last_row, frames;
    int matrix, range, siting;
    void *dst;
    int64_t dst_frame_stride;
};
// Frames in: frame i's planes at src + i * src_frame_stride, its pixels at dst + i * dst_frame_stride.  Replicate mode
// ignores the siting.
struct YuvInJob {
    const char *name;
    const void *src;
    int64_t src_frame_stride;
    int width, height, frames;
    int matrix, range, chroma, siting;
    void *dst;
    int64_t dst_frame_stride;
};
// Every check refuses by name in `err` and needs no GPU; every launcher checks first, and *path (may be null) receives 0
// for the aligned path, 1 for the other.  The refusals all share: a size below 1 x 1, no frame or more than 65 535, an
// unknown matrix or range, an unknown chroma mode (frames in), a siting that is neither.

// RGBA8 frames of a clip to planar Y'CbCr 4:2:0 in one launch (k_rgba8_to_yuv420_clip, clip_yuv.hip; mmhip_clip_to_yuv420
// and mmhip_clip_to_yuv420_sited state the semantics, mm_yuv.h holds the arithmetic).  The launcher takes the path of
// aligned wide accesses where the width is a multiple of 8, src and both source strides are multiples of 16 and dst and
// dst_frame_stride multiples of 8, else the path of byte accesses: the same bytes.  Refused next: rows outside the
// frame, an odd first_row, an odd last_row that is not the height, null pointers, a src_row_stride below one row, a
// dst_frame_stride below one frame, a Y plane or a source band beyond 4 GiB.  Timed through ws.timed_launch as yuv420_clip.
int check_rgba8_to_yuv420_clip(const YuvOutJob &job, std::string *err);
int launch_rgba8_to_yuv420_clip(const YuvOutJob &job, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err);
// Float frames of a clip (float4 RGBA, what floatmap = 1 lands) to planar Y'CbCr 4:2:0 with 10-bit samples in 16-bit
// words in one launch (k_float_to_yuv420p10_clip, clip_yuv10.hip; mmhip_clip_float_to_yuv420p10 and its _sited twin state
// the semantics, mm_yuv.h holds the arithmetic).  The aligned path where the width is a multiple of 8 and src, both source
// strides, dst and dst_frame_stride are multiples of 16, else the path of per-pixel loads and 2-byte stores: the same
// samples.  Refused next: what check_rgba8_to_yuv420_clip refuses, a source pointer or stride that is no multiple of 4,
// an odd dst or dst_frame_stride.  Timed through ws.timed_launch as yuv420p10_clip.
int check_float_to_yuv420p10_clip(const YuvOutJob &job, std::string *err);
int launch_float_to_yuv420p10_clip(const YuvOutJob &job, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err);
// Planar Y'CbCr 4:2:0 frames of a clip to drawable words in one launch (k_yuv420_to_rgba_clip, clip_yuv_in.hip;
// mmhip_clip_from_yuv420 and mmhip_clip_from_yuv420_sited state the semantics, mm_yuv.h holds the arithmetic).  The aligned
// path where the width is a multiple of 8, src and src_frame_stride are multiples of 8 and dst and dst_frame_stride
// multiples of 16, else the path of byte accesses: the same words.  Refused next: null pointers, a stride below one
// frame, a dst_frame_stride that is no multiple of 4, a destination frame beyond 4 GiB.  Timed through ws.timed_launch as
// yuv420_to_rgba_clip.
int check_yuv420_to_rgba_clip(const YuvInJob &job, std::string *err);
int launch_yuv420_to_rgba_clip(const YuvInJob &job, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err);
// Planar Y'CbCr 4:2:0 frames of 16-bit samples (10 bits used) to the float4 texels of a deep drawable in one launch
// (k_yuv420p10_to_float_clip, clip_yuv10_in.hip; mmhip_clip_from_yuv420p10 and its _sited twin state the semantics, mm_yuv.h
// holds the arithmetic).  The aligned path where the width is a multiple of 8 and src and src_frame_stride are multiples
// of 16, else the path of 2-byte loads and per-pixel stores: the same floats.  Refused next: what
// check_yuv420_to_rgba_clip refuses, an odd src or src_frame_stride, a dst or dst_frame_stride that is no multiple of
// 16.  Timed through ws.timed_launch as yuv420p10_to_float_clip.
int check_yuv420p10_to_float_clip(const YuvInJob &job, std::string *err);
int launch_yuv420p10_to_float_clip(const YuvInJob &job, NativeWorkspace &ws, hipStream_t s, int *path, std::string *err);

}  // namespace mm
