/*
 * mmhip.h -- C ABI of the MI355X-native MathMap pixel engine (libmathmap_hip.so).
 *
 * Standalone tier: compile a .mm filter, bind user values / input images, render
 * rows on the GPU.  Mirrors the life cycle of the reference's session API
 * (mathmap.h:274-299, mathmap_common.c):
 *
 *   mmhip_compile        ~ compile_mathmap        (mathmap_common.c:503-582)
 *   mmhip_invoke         ~ invoke_mathmap         (mathmap_common.c:746-795)
 *   mmhip_set_*          ~ -D name=value handling (mathmap_cmdline.c:756-796)
 *   mmhip_render         ~ invocation_new_frame + call_invocation_parallel_and_join
 *                          (mathmap_common.c:797-1018); one launch renders the row band
 *   mmhip_unload         ~ unload_mathmap / free_invocation
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * Every function returning int returns 0 on success and a negative value on
 * error; mmhip_last_error() then holds the message (the reference's error_string,
 * exprtree.c:40).  The reference-ABI tier (gen_and_load_hip_code) is declared in
 * mathmap_hip_backend.h.
 */
#ifndef MMHIP_H
#define MMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmhip_filter mmhip_filter;
typedef struct mmhip_invocation mmhip_invocation;

/* user value kinds (userval.h:34-42) */
enum { MMHIP_UV_INT = 0, MMHIP_UV_FLOAT = 1, MMHIP_UV_BOOL = 2, MMHIP_UV_COLOR = 3,
       MMHIP_UV_CURVE = 4, MMHIP_UV_GRADIENT = 5, MMHIP_UV_IMAGE = 6 };

/* edge behaviours (mathmap.h:134-147) */
enum { MMHIP_EDGE_COLOR = 0, MMHIP_EDGE_WRAP = 1, MMHIP_EDGE_REFLECT = 2, MMHIP_EDGE_ROTATE = 3 };

/* gaussian_blur's arithmetic (mmhip_options.gauss_mode) */
enum { MMHIP_GAUSS_EXACT = 0, MMHIP_GAUSS_TOLERANCE = 1 };

typedef struct mmhip_options {
    int intersample;      /* 1 = bilinear input sampling (CLI -i), 0 = nearest */
    int supersampling;    /* affects the nearest fetch only (builtins.c:154-158) */
    int edge_behaviour_x, edge_behaviour_y;
    int tile_w;           /* workgroup tile width in pixels: 8,16,32,64,128,256 (0 = default) */
    int specialize_uservals; /* 1 = JIT a kernel variant per set of scalar user values with the values baked
                                in as literals and the reference's literal folds applied (x*0 -> 0, x+0 -> x,
                                dead branches); off by default */
    int pixel_inc;        /* drawable_get_pixel_inc (mathmap.c:1320-1327): the stride of the preview's image source
                             (fast_image_source_scale) the bilinear fetch interpolates over (builtins.c:186-216);
                             0 or 1 = full-resolution sources, the CLI's and every final render's case */
    int gauss_mode;       /* MMHIP_GAUSS_EXACT (default): gaussian_blur's float map equals the reference's bit for bit.
                             MMHIP_GAUSS_TOLERANCE (an extension): a faster chain (fma recurrences, lines split into
                             segments) whose RGBA8 output differs from the exact chain's by at most 1 per channel (its
                             float values by a few f32 ulps), used only where nothing but those bytes leaves the blur:
                             the render writes RGBA8 straight from the blur (a filter like examples/Blur/Gaussian Blur.mm
                             at pixel centres) over the whole frame, the blur's map is not kept (the first render of an
                             argument set: the second is memoised and exact), the input is a drawable (not a float map, a
                             closure or another native result), and both deviations are at least 0.5 px.  Everything else
                             -- float-map output, row bands, stripes, supersampling, memoised maps -- runs the exact chain.
                             Not part of the kernel source.  Other values: mmhip_compile* fails. */
    int deep_inputs;      /* 1 (an extension): the filter's kernels can fetch float32 input drawables -- MM_IMG_DEEP images,
                             bound by mmhip_set_image_sequence_float_host / _device, where the semantics are stated.  Part of
                             the kernel source (#define MM_DEEP_INPUTS 1): with 0, the default, the generated text is what it
                             is without the option and the two setters refuse the filter.  Every other kind of image is
                             fetched as before either way.  Not together with pixel_inc > 1 (the preview's stride has no
                             meaning for these images).  Values other than 0 and 1: mmhip_compile* fails. */
    int reserved[4];
} mmhip_options;

typedef struct mmhip_userval_info {
    int kind;
    int index;
    char name[64];
    int int_min, int_max, int_default;
    float float_min, float_max, float_default;
    int bool_default;
    unsigned image_flags;
} mmhip_userval_info;

const char *mmhip_last_error(void);
const char *mmhip_version(void);

/* ---- compile (no GPU needed up to mmhip_filter_load) ---- */
void mmhip_default_options(mmhip_options *o);
mmhip_filter *mmhip_compile(const char *source, const mmhip_options *opts);
/* like mmhip_compile, with n scalar user values (index, value) baked in as literals */
mmhip_filter *mmhip_compile_specialized(const char *source, const mmhip_options *opts, int n, const int *indices,
                                        const double *values);
/* the variant of a compiled filter (from source text or from an IR dump) with n scalar user values baked in:
   what a render with those values runs when the filter was compiled with specialize_uservals */
mmhip_filter *mmhip_filter_specialized(const mmhip_filter *f, int n, const int *indices, const double *values);
/* builds a filter from an IR dump (the JSON of mmhip_filter_ir_json): IR-level entry point */
mmhip_filter *mmhip_compile_ir_json(const char *ir_json, const mmhip_options *opts);
void mmhip_filter_free(mmhip_filter *f);
const char *mmhip_filter_name(const mmhip_filter *f);
int mmhip_filter_num_uservals(const mmhip_filter *f);
int mmhip_filter_userval_info(const mmhip_filter *f, int index, mmhip_userval_info *out);
const char *mmhip_filter_ir_json(mmhip_filter *f);        /* IR dump after the optimisation passes */
/* IR dump straight out of lowering (or the reference-ABI importer), before constant specialisation,
   copy propagation / DCE, loop-carried CSE and frame-constant hoisting: the input of
   mmhip_compile_ir_json and of the test oracle (oracle/ccgen.py) */
const char *mmhip_filter_ir_json_raw(mmhip_filter *f);
const char *mmhip_filter_kernel_source(mmhip_filter *f);  /* the HIP C++ handed to hiprtc */
int mmhip_filter_gauss_mode(const mmhip_filter *f);       /* the options' gauss_mode the filter was compiled with */
int mmhip_filter_deep_inputs(const mmhip_filter *f);      /* the options' deep_inputs the filter was compiled with */
int mmhip_filter_num_native_calls(const mmhip_filter *f);
/* The builtin overloads and macros the parser resolved while it compiled the filter's text, callees included: their
   unique ids ("mul_quat", "div_s", "macro___origVal", ...), sorted, one per line, as a NUL-terminated string of at
   most cap bytes in buf (truncated where cap is smaller).  Returns the size that holds all of them, the NUL included;
   buf may be NULL to ask for it.  Overload resolution takes the first match, so this is how a caller learns which
   overload an expression reached.  Empty for a filter built from an IR dump.  Not part of the generated code. */
int mmhip_filter_builtin_ids(const mmhip_filter *f, char *buf, int cap);
/* The launch geometry of the filter's pixel kernel over rows [0, num_rows) of a region_w-wide region, as
   mmhip_render takes it (MMHIP_PPT included): out[MMHIP_GEOMETRY_FIELDS] receives, in this order,
   tiles_x, tiles_y, wg1 (workgroups at one row per work-item, the rows-per-item choice's input), nwg (workgroups
   launched), ppt (rows per work-item), tile_w, tile_h, unroll (MM_UNROLL), pair_mode, single_pixel, xcd_order,
   tiles_magic (0: plain division) and xcd_full (workgroups that XCD order 2 swizzles).  No GPU needed. */
enum { MMHIP_GEOMETRY_FIELDS = 13 };
int mmhip_filter_launch_geometry(const mmhip_filter *f, int region_w, int num_rows, int64_t *out);
/* closure images the filter renders whole (render_image's closure branch), and the geometry of closure #closure's
   own launch over a width x height frame (same fields) */
int mmhip_filter_num_closures(const mmhip_filter *f);
int mmhip_filter_closure_launch_geometry(const mmhip_filter *f, int closure, int width, int height, int64_t *out);
/* The same 13 fields for one frame of a clip render of `frames` frames (mmhip_render_clip): the rows-per-item choice
   is made from the workgroups of all frames together, so ppt grows with the clip's length; nwg and tiles_y are one
   frame's.  frames = 1 gives mmhip_filter_launch_geometry's values.  No GPU needed. */
int mmhip_filter_clip_launch_geometry(const mmhip_filter *f, int region_w, int num_rows, int frames, int64_t *out);
/* How mmhip_render_clip cuts such a clip into launches: out[MMHIP_CLIP_PLAN_FIELDS] receives grid_x (gridDim.x: nwg
   rounded up to a multiple of 8), frames_per_batch (gridDim.y of a full batch: at most 65 535, grid_x * frames * 256
   below 2^31, and no more than the environment's MMHIP_CLIP_MAX_FRAMES, which is read once; 0 where the clip is
   rendered frame by frame), batches (pixel launches of the call) and shared_slot (1: the frame constants do not read
   t or frame, one prologue serves every frame).  No GPU needed. */
enum { MMHIP_CLIP_PLAN_FIELDS = 4 };
int mmhip_filter_clip_batch_plan(const mmhip_filter *f, int region_w, int num_rows, int frames, int64_t *out);
/* The native batches of such a clip at render size render_w x render_h: out[MMHIP_CLIP_NATIVE_PLAN_FIELDS] receives
   eligible (1: every native call of the filter is a gaussian_blur the batches take, see mmhip_render_clip),
   frames_per_batch (the smallest of mmhip_filter_clip_batch_plan's cap, 65 535 jobs and MMHIP_CLIP_NATIVE_BYTES /
   bytes_per_frame; the environment variable is read once, default 8 GiB; 0: below 2, the clip is rendered frame by
   frame), batches, and bytes_per_frame (per call site the checkpoints, 8 B/px rounded up to blocks of 16 steps, the
   16 B/px intermediate and a 16 B/px map). */
enum { MMHIP_CLIP_NATIVE_PLAN_FIELDS = 4 };
int mmhip_filter_clip_native_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int render_h, int frames,
                                  int64_t *out);
/* The clip variant of the module -- kernels mm_prologue_clip, mm_rows_clip (filters with a per-row slice) and
   mm_pixels_clip: the text of mmhip_filter_kernel_source with the kernels' heads replaced -- and its gfx950 compile
   (like mmhip_filter_jit).  Built on the first clip render of the filter, cached on it and on disk. */
const char *mmhip_filter_clip_kernel_source(mmhip_filter *f);
long mmhip_filter_jit_clip(mmhip_filter *f, int load_module);
/* hiprtc-compiles for gfx950 and (if a device is present) loads the module.
   load_module = 0 only compiles (usable without a GPU).  Returns code size. */
long mmhip_filter_jit(mmhip_filter *f, int load_module);
double mmhip_filter_jit_seconds(const mmhip_filter *f);

/* ---- invocation ---- */
mmhip_invocation *mmhip_invoke(mmhip_filter *f, int img_width, int img_height);
void mmhip_invocation_free(mmhip_invocation *inv);
int mmhip_set_int(mmhip_invocation *inv, int index, int value);
int mmhip_set_float(mmhip_invocation *inv, int index, float value);
int mmhip_set_bool(mmhip_invocation *inv, int index, int value);
int mmhip_set_color(mmhip_invocation *inv, int index, float r, float g, float b, float a);
/* curve = 1024 samples of the transfer curve over [0,1]; gradient = 1024 packed 0xRRGGBBAA colours
   (USER_CURVE_POINTS / USER_GRADIENT_POINTS, userval.h:36-37).  Defaults: identity ramp, grey ramp. */
/* Row-striped frames with native-filter calls: allow native filters to fill only the rows a
   stripe render reads (+- margin rows, plus the filter's own halo).  -1 = whole map (default). */
int mmhip_set_native_row_margin(mmhip_invocation *inv, int margin);
int mmhip_set_curve(mmhip_invocation *inv, int index, const float *values1024);
int mmhip_set_gradient(mmhip_invocation *inv, int index, const uint32_t *rgba1024);
int mmhip_set_by_name(mmhip_invocation *inv, const char *name, const char *value);  /* -Dname=value */
/* Input image from host memory: channels = 3 (RGB8, alpha forced to 255 as
   mathmap_cmdline.c:183 does) or 4 (RGBA8).  Uploaded once, stays in HBM. */
int mmhip_set_image_host(mmhip_invocation *inv, int index, const uint8_t *pixels, int width, int height, int channels);
/* Input image already resident in HBM as packed 0xRRGGBBAA uint32 per pixel.  Not copied and not owned.
   Contents rewritten in place: the invocation keeps what it has read from a bound pointer -- frame constants such as
   in(xy:[0.1, 0.2]) while the prologue is skipped, native results while their memo answers -- and may go on using it
   for as long as the pointer stays bound.  Calling this setter (or the _sequence_ one) again, with the same pointer, once
   the writer's work has been waited for or ordered in front of the next render's stream, publishes the new contents to
   frame constants and native results alike; without that call a later render may show the old contents, the new ones,
   or both. */
int mmhip_set_image_device(mmhip_invocation *inv, int index, const void *device_rgba32, int width, int height);
/* Multi-frame input (an extension; the reference's drawables carry num_frames cache entries, mathmap_cmdline.c:131-184):
   num_frames frames of width x height, packed one after the other -- color_t[num_frames][height][width] in HBM, host
   pixels frame by frame in the single-image format.  The two setters above are the num_frames = 1 case.
     - in(xy, n) reads frame (int)n -- truncated toward zero as x86-64 converts it, so -0.5 is frame 0 and NaN or a value
       beyond int is none; plain in(xy) passes t and reads frame (int)t.  n may differ from pixel to pixel.
     - Per tap, in the reference's order: an unbound image is white; the edge behaviour is applied; x outside gives
       edge colour x; y outside edge colour y; then a frame outside [0, num_frames) gives opaque white.  An edge colour
       wins over a bad frame.
     - All frames have one size; scale and middle are those of one frame.
     - Native filters and render() sample ORIG_VAL(x, y, image, 0.0) (builtins.c:273-343 render_image): gaussian_blur(in, ..),
       convolve, render(in) and the direct RGBA8 blur output (exact and tolerance chains) read FRAME 0 of a sequence
       (the default; mmhip_set_native_input_frame makes it the render's own frame).
     - Float maps (native results, closure images) have one frame and ignore the frame number.
     - The reference-ABI tier (mathmap_hip_backend.h) binds one frame per drawable.
   Errors: num_frames < 1; a total byte count that overflows or cannot be allocated; height * num_frames of
   2^31 rows or more (the generic fetch counts the sequence's rows in an int).  Rebinding makes native results stale. */
int mmhip_set_image_sequence_host(mmhip_invocation *inv, int index, const uint8_t *pixels, int width, int height, int channels,
                                  int num_frames);
int mmhip_set_image_sequence_device(mmhip_invocation *inv, int index, const void *device_rgba32, int width, int height,
                                    int num_frames);
/* Float32 input drawables ("deep" images; an extension): texels are four floats, float4[num_frames][height][width] in HBM,
   frames one after the other -- the layout a whole-frame floatmap = 1 clip render writes with frame_stride = 16 * width *
   height, so that one filter's float frames are the next one's input without an 8-bit step.  Only for invocations of a
   filter compiled with mmhip_options.deep_inputs = 1.  Width, height, num_frames, scale and middle are those of an 8-bit
   drawable of the same size, and so is everything else of the invocation: clip paths, shutter, aa, reconstruction filters
   and pixel formats do not know the kind of an input.
   The fetch is the drawable fetch with the byte step taken out:
     - Coordinates exactly as for an 8-bit drawable: the resize factors, (x + middle_x) * scale_x and -((y - middle_y) *
       scale_y), + 0.5 unless supersampling, floor and the x86 conversion to int; for the bilinear fetch x1 = floor(x),
       x2 = x1 + 1, x2fact = x - (float)x1, x1fact = 1 - x2fact (y alike) and the weights p1fact = x1fact * y1fact,
       p2fact = x1fact * y2fact, p3fact = x2fact * y1fact, p4fact = x2fact * y2fact of taps (x1, y1), (x1, y2), (x2, y1),
       (x2, y2).
     - One tap, in the order of the 8-bit tap: an unbound image gives (1, 1, 1, 1); the edge behaviour is applied; x outside
       gives edge colour x; y outside edge colour y; then a frame outside [0, num_frames) gives (1, 1, 1, 1); otherwise
       the texel's four floats as stored.  Edge colours become floats as TUPLE_FROM_COLOR makes them (byte / 255).
     - No clamp and no rounding: NaN, +-inf, negative values, values above 1 and denormals pass through.
     - No texel is loaded before its bounds and frame tests have passed: no coordinate forms an address outside the
       sequence.
     - Nearest: the result is the tap.  Bilinear: per channel ((p1 * p1fact + p2 * p2fact) + p3 * p3fact) + p4 * p4fact,
       every product and sum one float32 operation rounded to nearest, in that order, none contracted to an fma; no rintf
       and no division by 255.  On texels that are bytes / 255 the result is therefore within 0.5 / 255 (the byte rounding
       the 8-bit fetch applies) plus a few float32 ulps of the 8-bit fetch's, not equal to it.
     - A coordinate that is NaN, infinite or at or beyond 2^31 px gives what the same formulas give (not pinned); the
       fetch stays inside the buffer.
   _host: `pixels` is float[num_frames][height][width][channels], channels 3 (alpha becomes 1.0f) or 4; uploaded once, owned
   by the invocation.  _device: `device_float4` is already in HBM, 16-byte aligned, not copied and not owned.
   Either replaces whatever was bound to the index, 8-bit or deep (an upload the invocation owned is freed), and an 8-bit
   setter replaces a deep image likewise.  Rebinding makes native results stale.
   Contents rewritten in place behind a bound _device pointer ("chain in HBM": one filter's float maps are the next one's
   drawable) follow the rule stated at mmhip_set_image_device: call the setter again with the same pointer to publish
   them to frame constants and native results; without that call the invocation may keep what it read.
   Native filters (gaussian_blur, convolve, half_convolve, visualize_fft, render()) read their image argument as bytes: a
   call whose argument is a deep image fails that render with a message that names the filter and says that float inputs are
   not supported there; the invocation stays usable.  A closure image whose body fetches a deep image is generated code and
   works.
   Errors, before anything is allocated or bound: width or height < 1; num_frames < 1; channels neither 3 nor 4; a null
   pointer, or a device pointer that is not 16-byte aligned; a byte count that overflows; height * num_frames of 2^31 rows
   or more (as for 8-bit sequences); a filter compiled without deep_inputs. */
int mmhip_set_image_sequence_float_host(mmhip_invocation *inv, int index, const float *pixels, int width, int height, int channels,
                                        int num_frames);
int mmhip_set_image_sequence_float_device(mmhip_invocation *inv, int index, const void *device_float4, int width, int height,
                                          int num_frames);
/* Which frame of a bound sequence native filters read (gaussian_blur, render(), convolve, half_convolve,
   visualize_fft; an extension).  The reference's render_image samples its argument at frame 0 (ORIG_VAL(fx, fy, image,
   0.0), builtins/builtins.c:334), so gaussian_blur(in, ...) on a sequence blurs frame 0 in every output frame:
     MMHIP_NATIVE_FRAME_ZERO (default)  that behaviour, byte for byte;
     MMHIP_NATIVE_FRAME_CURRENT         an argument that is a bound drawable of more than one frame is read at the
                                        render's own frame number (mmhip_render's `frame`, frames[i] of a clip): the
                                        native filter sees that frame as a single image.
   In `current` mode a render whose frame number the sequence does not have fails, with a message naming the filter and
   the frame; it never reads another frame instead.  Closure images keep the reference's rule (their body runs at frame
   0); in(xy, n) in filter code is not affected.  A result computed from one frame is never reused for another: the frame
   number is part of what the native results' memo compares.  Errors: a mode that is neither constant. */
enum { MMHIP_NATIVE_FRAME_ZERO = 0, MMHIP_NATIVE_FRAME_CURRENT = 1 };
int mmhip_set_native_input_frame(mmhip_invocation *inv, int mode);
/* The colours (0xRRGGBBAA) a fetch beyond the left / right and the upper / lower edge returns under edge behaviour
   "colour".  Frame constants follow a change (the colours are part of what the prologue skip compares), and so do
   native results: render(in) keeps the drawable's resize wrapper and samples a non-square drawable beyond its edges
   with these colours, so a change of either colour makes every native result stale.  Setting the colours they
   already have changes nothing and keeps the results. */
int mmhip_set_edge_colors(mmhip_invocation *inv, uint32_t color_x, uint32_t color_y);
int mmhip_set_render_size(mmhip_invocation *inv, int render_width, int render_height);
/* sub-pixel sampling offset of the slice (mathmap.h:219; -0.5 for the second supersampling pass) */
int mmhip_set_sampling_offset(mmhip_invocation *inv, float offset_x, float offset_y);

/* Renders rows [first_row, last_row) of region (region_x, region_y, region_w, region_h)
   at animation parameter t / frame into device memory `out_device` (row 0 of the
   band at out_device; bpp bytes per pixel, row_stride bytes per row; floatmap != 0
   writes float[4] per pixel instead -- its rows are the *frame's* render width apart,
   16 * render_width bytes, whatever the region's width and row_stride, like the
   reference's float-map bands (new_template.c.in:297); the region's columns sit at the
   start of each row).  `stream` is a hipStream_t (NULL = the invocation's own stream).
   Asynchronous. */
int mmhip_render(mmhip_invocation *inv, int frame, float t, int region_x, int region_y, int region_w, int region_h,
                 int first_row, int last_row, void *out_device, int row_stride, int bpp, int floatmap, void *stream);
/* Renders a clip (an extension): the rows [first_row, last_row) of the region for num_frames frames of an animation,
   frame i at animation parameters frames[i] / ts[i] into out_device + i * frame_stride.  Everything else is
   mmhip_render's; frame i receives exactly the bytes mmhip_render(inv, frames[i], ts[i], ...) writes.
     - frames and ts are host arrays of num_frames entries; they are copied before the call returns.  Frame numbers
       and t need be neither consecutive nor monotone.
     - frame_stride (bytes) is at least one frame's band -- (rows - 1) * row_stride + region_w * bpp, for float maps
       rows * 16 * render_width -- and otherwise free; bytes between the bands are not touched.
     - One prologue launch, one launch of the per-row slice (filters that have one) and one pixel launch render a whole
       batch of frames: at most 65 535 frames and 2^31 work-items per launch (mmhip_filter_clip_batch_plan), more frames
       become several batches on the same stream.  A filter whose frame constants do not read t or frame evaluates
       them once per call.
     - Filters that call native filters (gaussian_blur, ...) or render closure images need the host between the
       prologue and the pixels of every frame: for them the call is a loop of mmhip_render.  Nothing is refused;
       mmhip_clip_batched_launches tells the two apart.
     - ... except filters whose native calls are all gaussian_blur outside loops (no closure images, gauss_mode exact,
       MMHIP_GAUSS_SEGMENTS unset, no native row margin): one prologue launch over a batch, one read-back of its
       records, every distinct blur of a call site in one launch set over the frames, then the pixel launch over
       per-frame image tables -- or none, where the blurs write the frames' RGBA8 bytes themselves.  The bytes are the
       loop's.  A batch holding a call the batched blur does not take (a deviation below half a pixel, an input of
       another size or under a non-identity mapping) is rendered by the loop.  mmhip_filter_clip_native_plan and the
       mmhip_clip_native_* counters report this path; mmhip_clip_batched_launches and mmhip_clip_prologue_frames
       stay those of filters without native calls.
     - Asynchronous like mmhip_render.  With mmhip_enable_timing, mmhip_drain_kernel_ms reports one entry per batch.
     - Supersampled clips (the CLI's -o) are mmhip_render_clip_supersampled's: two of these calls and one combine per batch.
   Errors: num_frames < 1; frames or ts NULL; a frame_stride smaller than the band; mmhip_render's own. */
int mmhip_render_clip(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int region_x, int region_y,
                      int region_w, int region_h, int first_row, int last_row, void *out_device, int row_stride,
                      int64_t frame_stride, int bpp, int floatmap, void *stream);
/* Batched pixel launches (mm_pixels_clip) of this invocation so far: one per batch of a clip render, none for a
   filter mmhip_render_clip renders frame by frame.  mmhip_clip_prologue_frames: the frames whose frame constants the
   clip prologue evaluated (one per call where they do not read t or frame). */
long mmhip_clip_batched_launches(mmhip_invocation *inv);
long mmhip_clip_prologue_frames(mmhip_invocation *inv);
/* The native batches of clip renders so far (filters whose native calls are gaussian_blur): batches run, blurs computed
   in them (frames of a batch with equal arguments share one), and frames whose bytes a blur wrote itself (no pixel
   launch).  A batch that fell back to the loop counts in none of them. */
long mmhip_clip_native_batches(mmhip_invocation *inv);
long mmhip_clip_native_blurs(mmhip_invocation *inv);
long mmhip_clip_native_direct_frames(mmhip_invocation *inv);
/* The CLI's -o: supersampled render of a region (two slices + 1-1-2-1-1 / 6 byte combine,
   call_invocation, mathmap_common.c:880-927).  Compile the filter with supersampling = 1. */
int mmhip_render_supersampled(mmhip_invocation *inv, int frame, float t, int region_x, int region_y, int region_w,
                              int region_h, void *out_device, int row_stride, int bpp, void *stream);
/* A supersampled clip (an extension): frame i at out_device + i * frame_stride receives exactly the bytes
   mmhip_render_supersampled(inv, frames[i], ts[i], region..., row_stride, bpp, stream) writes; bytes between rows and
   between frames are not touched.  frames, ts, frame_stride and the errors are mmhip_render_clip's; asynchronous.
     - The clip is cut into batches.  Per batch: mmhip_render_clip of the long slices (region_w + 1 columns, sampling
       offsets -0.5) into a temporary of the invocation's whose rows are a multiple of 16 bytes apart, mmhip_render_clip
       of the short slices (offsets 0), and one launch of the combine over all frames of the batch -- two batched pixel
       launches and one combine where the loop makes three launches and two prologues per frame.  The invocation's own
       sampling offsets are put back on every return.
     - Frames per batch: what either slice's clip launch takes at once (mmhip_filter_clip_batch_plan's caps), at most
       65 535, and MMHIP_CLIP_SS_BYTES (read once, default 2 GiB) / bytes_per_frame, where bytes_per_frame = region_h *
       (long_pitch + region_w * bpp) and long_pitch is (region_w + 1) * bpp rounded up to 16.
     - Filters that call native filters or render closure images are not batched: for them the call is the loop of
       mmhip_render_supersampled (their nested renders share the native results between the two slices of a frame).
       Nothing is refused and the bytes are the same; mmhip_clip_supersampled_batches stays 0.
     - mmhip_clip_batched_launches rises by 2 per batch (the nested clip calls'), mmhip_clip_supersampled_batches by 1.
       With mmhip_enable_timing the pixel entries are the nested calls' and the combine is reported by
       mmhip_drain_native_kernel_ms as supersample_combine_clip. */
int mmhip_render_clip_supersampled(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts,
                                   int region_x, int region_y, int region_w, int region_h, void *out_device, int row_stride,
                                   int64_t frame_stride, int bpp, void *stream);
long mmhip_clip_supersampled_batches(mmhip_invocation *inv);
/* How mmhip_render_clip_supersampled renders `frames` frames of a region (needs no GPU).  out[] receives
   MMHIP_CLIP_SS_PLAN_FIELDS values: batched (0: the loop of mmhip_render_supersampled), frames_per_batch, batches,
   bytes_per_frame (the two slices of one frame in the temporary), long_pitch (bytes between the long slice's rows), and
   the rows_per_item and pixels_per_item of the combine kernel (a work-item combines pixels_per_item adjacent pixels
   over rows_per_item rows). */
enum { MMHIP_CLIP_SS_PLAN_FIELDS = 7 };
int mmhip_filter_clip_supersample_plan(const mmhip_filter *f, int region_w, int region_h, int bpp, int frames, int64_t *out);
/* A motion-blurred clip (an extension): every output frame is the mean of `samples` = K sub-samples spread over `span`
   units of t, rendered as float maps in HBM and averaged there by a combine kernel.  frames, ts, the region, the rows,
   out_device, row_stride, frame_stride, bpp, floatmap and stream are mmhip_render_clip's; asynchronous.
     - samples is 1 to MMHIP_SHUTTER_MAX_SAMPLES (256); span is any finite float, 0 and negative ones included.
     - Sub-sample j (0 <= j < K) of output frame i is what mmhip_render produces as a float map at frame number
       frames[i] -- the same for every j, so in(xy, frame) reads one frame of a sequence -- and at the time
       t_ij = (float)((double)ts[i] + ((double)span * (double)j) / (double)K): double arithmetic, the product before
       the quotient, one rounding to float.
     - Per pixel and channel, in f32, round to nearest, no fma, denormals kept: acc = f_0; acc = acc + f_j for j = 1 ..
       K - 1 in that order; m = acc * inv_k with inv_k = (float)(1.0 / (double)K).
     - m is stored as mmhip_render stores a pixel: without floatmap the pixel store's bytes at output_bpp 1 - 4 (CLAMP01,
       products in double, truncation, grey for bpp 1 and 2, alpha at bpp - 1 for bpp 2 and 4), rows row_stride apart;
       with floatmap the four floats, rows 16 * render_width bytes apart with the region's columns at the start of each
       row.  Bytes between rows and between frames are not touched.
     - samples = 1 is mmhip_render_clip: the call delegates before anything else.
     - Per batch of B output frames: one nested mmhip_render_clip of B * samples_per_pass float maps (frames[i] repeated,
       the times above, frame_stride = bytes_per_sample = rows * 16 * render_width) into a temporary of the
       invocation's, then one launch of the combine on the same stream.  The nested call batches, runs native filters
       and closures and picks specialised variants as it always does: nothing is refused that mmhip_render_clip takes.
     - MMHIP_CLIP_SHUTTER_BYTES (read once, default 8 GiB) bounds the temporary.  Where the K sub-samples of one frame
       fit: frames_per_batch = min(budget / (K * bytes_per_sample), 65 535, num_frames) and one pass.  Otherwise one
       frame per batch in passes of samples_per_pass = max(1, budget / bytes_per_sample - 1) sub-samples, the running
       sum carried from pass to pass in one more float map; the order of the sum, and so its bits, are the same.  One
       sub-sample and the carry map are allocated even where they exceed the budget.
     - The invocation's state (memo, native maps, sampling offsets, the counters of other paths) is left as the nested
       clip calls leave it.  mmhip_clip_shutter_batches rises by one per batch; with mmhip_enable_timing the combine is
       reported by mmhip_drain_native_kernel_ms as shutter_combine_clip, once per pass.
     - Not combined with supersampling: there is no motion-blurred mmhip_render_clip_supersampled.
   Errors: samples out of range; a span that is not finite; a sub-sample map beyond 4 GiB; out of device memory (the
   message names MMHIP_CLIP_SHUTTER_BYTES); mmhip_render_clip's own. */
enum { MMHIP_SHUTTER_MAX_SAMPLES = 256, MMHIP_CLIP_SHUTTER_PLAN_FIELDS = 6 };
int mmhip_render_clip_shutter(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples, float span,
                              int region_x, int region_y, int region_w, int region_h, int first_row, int last_row,
                              void *out_device, int row_stride, int64_t frame_stride, int bpp, int floatmap, void *stream);
long mmhip_clip_shutter_batches(mmhip_invocation *inv);
/* How mmhip_render_clip_shutter renders `frames` frames of num_rows rows at render width render_w with `samples`
   sub-samples (needs no GPU).  out[] receives MMHIP_CLIP_SHUTTER_PLAN_FIELDS values: frames_per_batch, batches,
   samples_per_pass, passes (per frame), bytes_per_sample and carry (1: a carry map joins the passes). */
int mmhip_filter_clip_shutter_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int samples, int frames,
                                   int64_t *out);
/* The same motion-blurred clip without the sub-sample maps (an extension, opt-in): a variant of the pixel kernel,
   mm_pixels_shutter, evaluates the K sub-samples of an output pixel one after the other and sums them in registers.
   The parameters are mmhip_render_clip_shutter's, and so are the bytes: float maps bit for bit, bytes at bpp 1 - 4,
   nothing touched between rows or frames.  Asynchronous.
     - The sub-sample times, the order of the sum and the product with inv_k are those stated above (the JIT compiles
       without fma contraction); RAND's call counter starts at 0 in every sub-sample, as in a render of its own.
     - samples = 1 is mmhip_render_clip: the call delegates before anything else.  The 4 GiB limit of a sub-sample
       map does not apply: there is none, and no temporary is allocated.
     - Fused are filters without native calls and without closure images whose frame fits one launch (a batch of at
       least one frame, below).  For every other filter the call is mmhip_render_clip_shutter: nothing is refused, and
       mmhip_clip_shutter_fused_batches stays where it was.  The variant that renders (the filter, or its specialised
       variant for the current user values) has a shutter module of its own, built on the first such call.
     - mm_pixels_shutter always has the single-pixel shape (one pixel per work-item, the generic fetch) whatever the
       shape of the filter's pixel kernel: no pair mode, no unrolled hot fetch.
     - Per batch of B output frames: the {t, frame} table of all num_frames * K sub-samples goes up once per call; one
       launch of mm_prologue_clip (and mm_rows_clip) over the batch's B * K slots -- one slot for the whole call where the
       frame constants read neither t nor frame --, one launch of mm_pixels_shutter over (grid_x, B).
     - B is the largest value with B * K <= 65 535, B * K <= MMHIP_CLIP_MAX_FRAMES (read once), grid_x * B * 256 < 2^31,
       B <= num_frames and, where slots are per sub-sample, B * K slots of frame constants (and of row-table floats)
       within INT32_MAX.  grid_x is the workgroups of the region at one row per work-item, rounded up to a multiple of 8.
     - mmhip_clip_shutter_fused_batches rises by one per batch and mmhip_clip_prologue_frames by the slots launched;
       mmhip_clip_batched_launches, mmhip_clip_shutter_batches and the native counters do not move.  With
       mmhip_enable_timing, mmhip_drain_kernel_ms reports one entry per batch.
   Errors: those of mmhip_render_clip_shutter but the 4 GiB one, under the name render_clip_shutter_fused. */
int mmhip_render_clip_shutter_fused(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples,
                                    float span, int region_x, int region_y, int region_w, int region_h, int first_row,
                                    int last_row, void *out_device, int row_stride, int64_t frame_stride, int bpp, int floatmap,
                                    void *stream);
long mmhip_clip_shutter_fused_batches(mmhip_invocation *inv);
/* How mmhip_render_clip_shutter_fused renders `frames` frames of num_rows rows of a region_w-wide region with `samples`
   sub-samples (needs no GPU).  out[] receives MMHIP_CLIP_SHUTTER_FUSED_PLAN_FIELDS values: fused (0: the call is
   mmhip_render_clip_shutter, and the other fields but grid_x are 0), frames_per_batch (B), batches, slots_per_batch (B * K,
   or 1 where one slot serves the whole call) and grid_x. */
enum { MMHIP_CLIP_SHUTTER_FUSED_PLAN_FIELDS = 5 };
int mmhip_filter_clip_shutter_fused_plan(const mmhip_filter *f, int region_w, int num_rows, int samples, int frames, int64_t *out);
/* The shutter variant of the module -- mm_prologue_clip and mm_rows_clip as in the clip variant, and mm_pixels_shutter --
   and its gfx950 compile (like mmhip_filter_jit_clip; load_module = 0 needs no GPU).  Generated from the filter's code
   when first asked for, cached on the filter and on disk under its own key; the texts of mmhip_filter_kernel_source and
   mmhip_filter_clip_kernel_source stay what they were.  A filter with native calls or closure images has none: NULL and
   -1, with a message. */
const char *mmhip_filter_shutter_kernel_source(mmhip_filter *f);
long mmhip_filter_jit_shutter(mmhip_filter *f, int load_module);
/* A grid-supersampled clip (an extension): anti-aliasing in space, alone or together with a shutter.  Every output
   pixel is the mean of samples * grid_x * grid_y = K * G float sub-samples: K instants of the shutter, and at each of them
   a regular grid of sx = grid_x by sy = grid_y sampling offsets inside the pixel's footprint.  The parameters before and
   behind samples, span, grid_x, grid_y are mmhip_render_clip_shutter's; asynchronous.  (The CLI's -o,
   mmhip_render_clip_supersampled, is something else and stays what it is: the reference's five-tap average of bytes.)
     - samples = K is 1 to 256 and span any finite float, as for the shutter; grid_x and grid_y are 1 to
       MMHIP_SAMPLE_GRID_MAX (8) each; K * G is at most MMHIP_SHUTTER_MAX_SAMPLES (256).
     - The offsets (mathmap_amd/csrc/mm_sample_grid.h), in the units of mmhip_set_sampling_offset (pixels):
       ox_a = (float)(((double)a + 0.5) / (double)sx - 0.5) for a = 0 .. sx - 1, and oy_b the same with sy.  One point per
       axis is exactly 0.
     - Sub-sample (j, b, a) of output frame i is the float map mmhip_render produces at frame number frames[i], at the time
       t_ij of mmhip_render_clip_shutter (mm_shutter_sample_t(ts[i], span, j, K)) and at sampling offset (ox_a, oy_b).
       Native filters and closure renders see what they see in any render at that offset (closures render at offset 0).
     - Order and arithmetic: the sub-samples are numbered s = j * G + b * sx + a, a fastest.  Per pixel and channel, in f32,
       round to nearest, no fma: acc = f_0; acc = acc + f_s for s = 1 .. K * G - 1 in that order; m = acc * inv_k with
       inv_k = (float)(1.0 / (double)(K * G)).  m is stored as mmhip_render stores a pixel (bytes at bpp 1 - 4, or the
       float map).  These are the shutter's rules with K * G in place of K.
     - The call's grid offsets replace the invocation's sampling offset for the length of the call; the caller's offset is
       put back on every return, failed calls included.  Bytes between rows and between frames are not touched.
     - grid_x = grid_y = 1 is mmhip_render_clip_shutter: the call delegates before anything else (and samples = 1 then
       reaches mmhip_render_clip).
     - Per batch of B output frames and per pass of `count` time steps: for every grid point g = b * sx + a one nested
       mmhip_render_clip of the B * count (frame, t) entries at offset (ox_a, oy_b), into the shutter's temporary at
       g * bytes_per_sample with frame_stride G * bytes_per_sample -- entry e = i * count + j lands at (e * G + g) *
       bytes_per_sample, the layout [i][j][g] -- and then one launch of the shutter's combine over count * G samples.
       Nothing is refused that mmhip_render_clip takes.  Known cost: a filter with native calls runs them once per nested
       call, G times per batch.
     - MMHIP_CLIP_SHUTTER_BYTES bounds the temporary as it does for the shutter.  Where a frame's K * G maps fit:
       frames_per_batch = min(budget / (K * G * bytes_per_sample), 65 535, num_frames), one pass.  Otherwise one frame per
       batch in passes of whole time steps, steps_per_pass = max(1, (budget / bytes_per_sample - 1) / G), the running sum
       carried in one more map; one time step's G maps and the carry map are allocated even over the budget.
     - mmhip_clip_sampled_batches rises by one per batch; the shutter's counters do not move.  The combine is timed as
       shutter_combine_clip.
   Errors: a grid outside 1 .. 8; samples out of range; K * G > 256; a span that is not finite; a sub-sample map beyond
   4 GiB; out of device memory; mmhip_render_clip's own. */
enum { MMHIP_SAMPLE_GRID_MAX = 8, MMHIP_CLIP_SAMPLED_PLAN_FIELDS = 6 };
int mmhip_render_clip_sampled(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples, float span,
                              int grid_x, int grid_y, int region_x, int region_y, int region_w, int region_h, int first_row,
                              int last_row, void *out_device, int row_stride, int64_t frame_stride, int bpp, int floatmap,
                              void *stream);
long mmhip_clip_sampled_batches(mmhip_invocation *inv);
/* How mmhip_render_clip_sampled renders such a clip (needs no GPU).  out[] receives MMHIP_CLIP_SAMPLED_PLAN_FIELDS
   values: frames_per_batch, batches, steps_per_pass (time steps, of G maps each), passes (per frame), bytes_per_sample
   and carry. */
int mmhip_filter_clip_sampled_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int samples, int grid_x,
                                   int grid_y, int frames, int64_t *out);
/* The same clip without the sub-sample maps (opt-in): kernel mm_pixels_sampled of a variant of its own evaluates the
   K * G sub-samples of an output pixel one after the other and sums them in registers, in the order stated above.  The
   parameters and the bytes are mmhip_render_clip_sampled's.  Asynchronous.
     - grid_x = grid_y = 1 is mmhip_render_clip_shutter_fused: the call delegates before anything else.
     - mm_pixels_sampled has mm_pixels_shutter's shape (one work-item per output pixel, the generic fetch).  The slot
       i * K + j selects {t, frame} and the frame constants; x and y of grid point (a, b) come from per-offset coordinate
       tables -- sx * region_w and sy * rows floats -- which the variant's mm_prologue_clip writes with the expressions
       of every prologue, at the offsets of mm_sample_grid.h uploaded behind the {t, frame} table.
     - Fused are filters without native calls, without closure images and without a per-row slice (its values follow y;
       such filters take the maps path) whose frame fits one launch.  For every other filter the call is
       mmhip_render_clip_sampled: nothing is refused, and mmhip_clip_sampled_fused_batches stays where it was.
     - Batches are mmhip_render_clip_shutter_fused's: B * K slots per launch.  mmhip_clip_sampled_fused_batches rises by
       one per batch and mmhip_clip_prologue_frames by the slots launched; no other counter moves.
   Errors: those of mmhip_render_clip_sampled but the 4 GiB one, under the name render_clip_sampled_fused. */
int mmhip_render_clip_sampled_fused(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples,
                                    float span, int grid_x, int grid_y, int region_x, int region_y, int region_w, int region_h,
                                    int first_row, int last_row, void *out_device, int row_stride, int64_t frame_stride, int bpp,
                                    int floatmap, void *stream);
long mmhip_clip_sampled_fused_batches(mmhip_invocation *inv);
/* How mmhip_render_clip_sampled_fused renders such a clip (needs no GPU): the fields of
   mmhip_filter_clip_shutter_fused_plan (fused 0: the call is mmhip_render_clip_sampled). */
enum { MMHIP_CLIP_SAMPLED_FUSED_PLAN_FIELDS = 5 };
int mmhip_filter_clip_sampled_fused_plan(const mmhip_filter *f, int region_w, int num_rows, int samples, int grid_x, int grid_y,
                                         int frames, int64_t *out);
/* The sampled variant of the module -- mm_prologue_clip (with the per-offset tables) and mm_pixels_sampled -- and its gfx950
   compile, like mmhip_filter_shutter_kernel_source and mmhip_filter_jit_shutter: generated when first asked for, cached
   under its own key, the other three texts untouched.  A filter with native calls, closure images or a per-row slice has
   none: NULL and -1, with a message. */
const char *mmhip_filter_sampled_kernel_source(mmhip_filter *f);
long mmhip_filter_jit_sampled(mmhip_filter *f, int load_module);
/* An adaptively anti-aliased clip (an extension, opt-in): the grid-supersampled clip of mmhip_render_clip_sampled at
   samples = 1, refined only where a single-sample render shows contrast.  Every output pixel equals one of two existing
   renders, chosen by a mask computed from an existing render.  frames, ts, the region, the rows, out_device, row_stride,
   frame_stride, bpp, floatmap and stream are mmhip_render_clip's; asynchronous.  Spatial only: there is no shutter.
     - threshold is any float but NaN, which is refused before anything else is looked at.  mode is MMHIP_AA_REFINE_AUTO (0)
       or MMHIP_AA_REFINE_SELECT (1: force the select path, below).  grid_x and grid_y are mmhip_render_clip_sampled's.
     - grid_x = grid_y = 1 is mmhip_render_clip: the call delegates right after the threshold check.
     - For every frame i, F is the float map mmhip_render_clip(floatmap = 1) produces for (frames[i], ts[i]) at sampling
       offset (0, 0), whatever the invocation's offset, which is put back on every return, failed calls included.  The
       rendered rectangle is the region's columns by the rows [first_row, last_row) clamped to the region.
     - Clamp: c(v) = v < 0 ? 0 : (v > 1 ? 1 : v) in f32 -- NaN stays NaN, +inf becomes 1 and -inf 0.
     - Pixel p is refined iff threshold < 0, or some 8-neighbour q of p inside the rendered rectangle and some channel ch
       of the four give !(fabsf(c(F[p][ch]) - c(F[q][ch])) <= threshold): one f32 subtraction, no fma; a NaN contrast
       refines.  Neighbours outside the rectangle are skipped, so a 1 x 1 rectangle is refined by a negative threshold only.
     - A refined pixel receives exactly the bytes (or floats) mmhip_render_clip_sampled(samples = 1, grid_x, grid_y) gives
       it: all G = grid_x * grid_y grid points evaluated afresh (F is not reused), summed in the order b * sx + a, scaled by
       mm_shutter_inv_k(G), stored as mm_store_pixel stores.
     - Every other pixel receives what the shutter combine stores for the single sample F[p]: acc = f_0, times
       mm_shutter_inv_k(1), through mm_shutter_store_bytes at bpp 1 - 4 or as the four floats of a float map.
     - Known property: the mask looks at the rendered rectangle only, so a frame rendered in row bands refines differently
       at the band seams than a frame rendered whole.
     - List path (auto mode; filters mmhip_render_clip_sampled_fused takes: no native calls, no closure images, no per-row
       slice, a frame that fits one launch; region_w and rows at most 65 535), per batch of B frames: the nested
       mmhip_render_clip of the B base maps at offset 0, one launch of the mask kernel (k_aa_contrast_clip: it stores the
       pixels that are not refined, counts the refined ones per frame and appends them to the frame's list as
       col | rl << 16, in no particular order), the refine variant's mm_prologue_clip, and mm_pixels_refine over a grid
       of refine_grid_x = ceil(region_w * rows / 256) by B workgroups -- sized for the whole rectangle: the host never
       reads a count while rendering, and work-items beyond a frame's count return.
     - Select path (every other filter, larger regions, mode 1), per batch: the base maps, the nested
       mmhip_render_clip_sampled(samples = 1) of the same frames into out_device, and the mask kernel without lists, which
       overwrites the pixels that are not refined.  It saves no time; it exists so that nothing is refused and so that
       one filter can be rendered both ways.
     - Memory: B base maps of rows * 16 * render_width bytes and, on the list path, B lists of 4 bytes per pixel of the
       rectangle, in a temporary of the invocation's under MMHIP_CLIP_SHUTTER_BYTES: frames_per_batch = min(max(1, budget
       / bytes_per_frame), 65 535, num_frames) and, on the list path, at most the frames_per_batch of
       mmhip_filter_clip_sampled_fused_plan at samples = 1.  One frame is allocated even over the budget.  (The nested
       grid-supersampled clip of the select path has the shutter's temporary besides.)
     - mmhip_clip_adaptive_batches rises by one per batch.  No other counter moves but those the nested calls move
       themselves (the refine prologue is not counted in mmhip_clip_prologue_frames).  With mmhip_enable_timing the mask
       launch is reported by mmhip_drain_native_kernel_ms as aa_contrast_clip and mm_pixels_refine by
       mmhip_drain_kernel_ms, one entry per batch.
   Errors: a NaN threshold; a grid outside 1 .. 8 or of more than 256 points; a mode that is neither constant; a base map
   beyond 4 GiB; out of device memory; mmhip_render_clip's own. */
enum { MMHIP_AA_REFINE_AUTO = 0, MMHIP_AA_REFINE_SELECT = 1, MMHIP_CLIP_ADAPTIVE_PLAN_FIELDS = 5 };
int mmhip_render_clip_adaptive(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int grid_x, int grid_y,
                               float threshold, int mode, int region_x, int region_y, int region_w, int region_h, int first_row,
                               int last_row, void *out_device, int row_stride, int64_t frame_stride, int bpp, int floatmap,
                               void *stream);
long mmhip_clip_adaptive_batches(mmhip_invocation *inv);
/* The refined pixels of every frame of the last mmhip_render_clip_adaptive call of this invocation: counts[i] for
   i < min(n, frames of that call).  Waits for that call's stream.  Returns the frames of that call (0 after a call that
   delegated to mmhip_render_clip), or -1. */
int mmhip_clip_adaptive_refined(mmhip_invocation *inv, int64_t *counts, int n);
/* How mmhip_render_clip_adaptive renders `frames` frames in auto mode (needs no GPU).  out[] receives
   MMHIP_CLIP_ADAPTIVE_PLAN_FIELDS values: list_path (0: the select path), frames_per_batch, batches, bytes_per_frame (the
   base map and, on the list path, the list) and refine_grid_x (0 on the select path). */
int mmhip_filter_clip_adaptive_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int grid_x, int grid_y,
                                    int frames, int64_t *out);
/* The refine variant of the module -- the sampled variant's mm_prologue_clip, text unchanged, and mm_pixels_refine, which
   is mm_pixels_sampled with the tile order replaced by a read of the frame's list -- and its gfx950 compile, like
   mmhip_filter_sampled_kernel_source and mmhip_filter_jit_sampled: generated when first asked for, cached under its own
   key, the other four texts untouched.  A filter with native calls, closure images or a per-row slice has none: NULL and
   -1, with a message. */
const char *mmhip_filter_refine_kernel_source(mmhip_filter *f);
long mmhip_filter_jit_refine(mmhip_filter *f, int load_module);
/* A grid-supersampled clip under a reconstruction filter wider than a pixel (an extension, opt-in): every output pixel
   is a weighted sum of the sub-samples of its own grid and of the grids of its neighbour pixels, the weights a separable
   box, tent, Gaussian or Mitchell-Netravali kernel.  Every parameter except `kernel` and `radius` means what it means
   for mmhip_render_clip_sampled; asynchronous.  This statement is the specification: tests/clip_filter_reference.py
   restates it, mathmap_amd/csrc/mm_clip_filter.h holds it.
     - kernel is MMHIP_AA_BOX, MMHIP_AA_TENT, MMHIP_AA_GAUSSIAN or MMHIP_AA_MITCHELL.  radius is in pixels, finite, and
       0.5 <= radius <= 4.  The Python and CLI layers use these radii when none is given: box 0.5, tent 1.0, Gaussian 1.5,
       Mitchell 2.0.  D = (int)ceil(radius - 0.5) is the number of neighbour pixels reached on each side: 0 <= D <= 4.
     - samples, span, grid_x = sx, grid_y = sy, the offsets ox_a and oy_b, the sub-sample (j, b, a) of a pixel and its time
       t_ij are mmhip_render_clip_sampled's: sx and sy are 1 to 8, samples * sx * sy is at most 256.  A 1 x 1 grid is allowed:
       a post-filter of single samples.  Nothing delegates to another entry point.
     - Sample position: offsets add to the pixel index in both axes, so sub-sample (b, a) of the pixel at column c + dx, row
       r + dy lies, in double, at d_x = (double)dx + (double)ox_a and d_y = (double)dy + (double)oy_b from the centre of
       pixel (c, r).
     - The weight of one axis, k(d), in double, with ad = fabs(d) and R = (double)radius: 0 where ad >= R; else
         box: 1.0
         tent: 1.0 - ad / R
         Gaussian: exp(-2.0 * (d * d)) - exp(-2.0 * (R * R)), exp being the host libm's double function
         Mitchell (B = C = 1/3), with u = (2.0 * ad) / R:
           u < 1: (((7.0 * u - 12.0) * u) * u + 16.0 / 3.0) / 6.0
           else:  ((((-7.0 / 3.0) * u + 12.0) * u - 20.0) * u + 32.0 / 3.0) / 6.0
       each evaluated in the order written, without fma.
     - Taps: a tap of the x axis is a pair (dx, a) with dx = -D .. D and a = 0 .. sx - 1, in the order dx ascending, then a
       ascending.  It exists only where the neighbour pixel lies inside the frame: 0 <= region_x + c + dx < render_width;
       likewise (dy, b) and rows against render_height.  The frame counts, not the region and not the rows asked for: row
       bands and sub-regions of a call equal the same pixels of a whole-frame call.
     - Normalisation is per axis and per column (or row) of the frame: n is the double sum of k over the existing taps in
       tap order (n = 0.0; n = n + k), and the tap's weight is w = (float)(k / n).  A tap with w == 0 is dropped: it is
       never read, whatever it holds.  An n that is not a positive finite number refuses the call.  Only the first and last D
       columns and rows differ from the interior: a pixel with lo = min(D, index) neighbours before it and hi = min(D, size -
       1 - index) after it has the table of class (lo, hi), at most (D + 1)^2 tables per axis; they are built on the host
       and uploaded.  mmhip_clip_filter_taps returns one.
     - Arithmetic, per channel, in f32, round to nearest, no fma, denormals kept.  With f[g] the float map of grid point g
       = b * sx + a of a time step: h_b(c, r') is the sum over the taps (dx ascending, then a ascending) of wx * f[b * sx +
       a](c + dx, r') -- each product rounded on its own; the first product starts the sum, every later product is added to
       it in order.  s_j(c, r) is the same sum over (dy ascending, then b ascending) of wy * h_b(c, r + dy).  Over the K =
       samples time steps: acc = s_0; acc = acc + s_j for j = 1 .. K - 1; m = acc * (float)(1.0 / (double)K).
     - m is stored as every clip path stores a pixel: mm_shutter_store_bytes at bpp 1 - 4, or the float map.  Bytes
       between rows and between frames are not touched.  Box at radius 0.5 is not bit-identical to
       mmhip_render_clip_sampled in general: the association of the sum differs.
     - The sub-sample maps hold the haloed rectangle: columns [max(0, region_x - D), min(render_width, region_x + region_w
       + D)) by rows [max(0, first_row - D), min(render_height, last_row + D)).  Per batch and pass, for every grid point
       one nested mmhip_render_clip of that rectangle as float maps at the grid point's sampling offset, in the layout
       [i][j][g] of mmhip_render_clip_sampled, then one launch of the combine (k_filter_combine_clip).  Native filters and
       closures run as they do there; nothing that mmhip_render_clip accepts is refused.
     - Batches and passes are mmhip_render_clip_sampled's with the haloed row count in place of the rows:
       MMHIP_CLIP_SHUTTER_BYTES bounds the temporary, passes are whole time steps, and the carry map holds the running acc of
       the output rectangle.
     - The caller's sampling offset is put back on every return, failed calls included.  One upload of the tap tables per
       call, one combine launch per pass.  mmhip_clip_filtered_batches rises by one per batch; the sampled, shutter and
       adaptive counters do not move.  The combine is timed as filter_combine_clip.
   Errors: what mmhip_render_clip_sampled refuses, under the name render_clip_filtered; an unknown kernel; a radius
   outside the range; a region that does not lie inside the render size (0 <= region_x, region_x + region_w <=
   render_width, the rows inside [0, render_height) after the usual clamp); a sub-sample map of the haloed rectangle
   beyond 4 GiB; out of device memory. */
enum { MMHIP_AA_BOX = 0, MMHIP_AA_TENT = 1, MMHIP_AA_GAUSSIAN = 2, MMHIP_AA_MITCHELL = 3, MMHIP_CLIP_FILTERED_PLAN_FIELDS = 8 };
int mmhip_render_clip_filtered(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples, float span,
                               int grid_x, int grid_y, int kernel, float radius, int region_x, int region_y, int region_w,
                               int region_h, int first_row, int last_row, void *out_device, int row_stride, int64_t frame_stride,
                               int bpp, int floatmap, void *stream);
long mmhip_clip_filtered_batches(mmhip_invocation *inv);
/* How mmhip_render_clip_filtered renders the rows [first_row, last_row) of the columns [region_x, region_x + region_w) of
   a render_w x render_h frame (needs no GPU; the kernel does not matter, the radius does).  out[] receives
   MMHIP_CLIP_FILTERED_PLAN_FIELDS values: the six of mmhip_filter_clip_sampled_plan -- bytes_per_sample being a map of the
   haloed rectangle -- then halo_columns and halo_rows, the rectangle's size. */
int mmhip_filter_clip_filtered_plan(const mmhip_filter *f, int region_x, int region_w, int first_row, int last_row, int render_w,
                                    int render_h, int samples, int grid_x, int grid_y, float radius, int frames, int64_t *out);
/* The normalised float taps of one axis with n grid points, for a pixel with lo neighbours before it and hi after it
   inside the frame (0 <= lo, hi <= D; needs no GPU): out[(dx + D) * n + a] is the weight of tap (dx, a), 0 for a tap that
   does not exist.  Returns the number of floats written, (2 D + 1) * n, or -1. */
int mmhip_clip_filter_taps(int kernel, float radius, int n, int lo, int hi, float *out);
/* A clip as planar Y'CbCr 4:2:0: converts num_frames RGBA8 frames in device memory -- what every clip entry point above
   leaves at output_bpp 4 -- to the payloads of a YUV4MPEG2 file, on the GPU (k_rgba8_to_yuv420_clip, one launch).
   Asynchronous on `stream` (0: the invocation's), like mmhip_render_clip with out_device.  This statement is the
   specification: tests/yuv_reference.py restates it, mathmap_amd/csrc/mm_yuv.h holds it.
     - Source: frames of width x height RGBA8 pixels (4 bytes per pixel only), of which the rows [first_row, last_row) are
       converted.  src_rgba points at row first_row of frame 0; rows are src_row_stride bytes apart (at least 4 * width),
       frames src_frame_stride.  The alpha byte is not read, as the PNG writer drops it.
     - Destination: every frame is one contiguous Y4M payload: the Y plane, width * height bytes with rows `width` apart,
       then Cb, then Cr, each cw * ch bytes with cw = (width + 1) >> 1 and ch = (height + 1) >> 1, rows cw apart.  Frames
       are dst_frame_stride bytes apart, at least width * height + 2 * cw * ch (mmhip_yuv420_frame_bytes).  dst is the
       base of frame 0's whole-frame layout, for a row band too.
     - A band writes the Y rows [first_row, last_row) and the chroma rows [first_row / 2, (last_row + 1) / 2) and nothing
       else: no byte between frames, of other rows or behind the planes.  first_row must be even and last_row even or
       equal to height; under these two rules bands converted separately give the bytes of a whole-frame call.
     - Arithmetic: all int32, every / a floor division (an arithmetic shift of a signed value).  Per pixel
         Y = ((yr * R + yg * G + yb * B + 2^15) >> 16) + off
       Per chroma sample (cx, cy), with Rs, Gs, Bs the sums over the four pixels (min(2 cx + i, width - 1), min(2 cy + j,
       height - 1)), i, j in {0, 1} -- an odd last column or row is replicated; chroma is sited at the centre of the
       block, hence C420jpeg --
         Cb = clamp(((cbr * Rs + cbg * Gs + cbb * Bs + 2^17) >> 18) + 128, 0, 255)
         Cr likewise with crr, crg, crb.
       The clamp matters at full range only, where pure blue and pure red give 256.
     - Coefficients: floor(k * 2^16 + 0.5) of the standard's constants, the green luma coefficient and one chroma
       coefficient per row set so that each row sums exactly (white is Y 235 or 255, grey has chroma 128):
         matrix, range    off   yr, yg, yb            cbr, cbg, cbb            crr, crg, crb
         bt601 limited    16    16829, 33039, 6416    -9714, -19071, 28785     28784, -24103, -4681
         bt601 full       0     19595, 38470, 7471    -11058, -21710, 32768    32768, -27439, -5329
         bt709 limited    16    11966, 40254, 4064    -6596, -22189, 28785     28784, -26145, -2639
         bt709 full       0     13933, 46871, 4732    -7509, -25259, 32768     32768, -29763, -3005
       The Python and CLI layers use bt709 limited when nothing is given.
     - The kernel has a path of aligned wide accesses (width a multiple of 8, src_rgba and both source strides multiples
       of 16, dst and dst_frame_stride multiples of 8) and a path of byte accesses for everything else; the launcher
       chooses, the bytes are the same.  Timed as yuv420_clip (mmhip_drain_native_kernel_ms).
   Errors, by name: width or height below 1; num_frames below 1 or above 65 535; an unknown matrix or range; rows that
   are not rows of the frame; an odd first_row; an odd last_row that is not height; a src_row_stride below one row; a
   dst_frame_stride below one frame; a Y plane or a source band of more than 4 GiB (offsets inside a frame are 32-bit). */
enum { MMHIP_YUV_BT601 = 0, MMHIP_YUV_BT709 = 1 };
enum { MMHIP_YUV_LIMITED = 0, MMHIP_YUV_FULL = 1 };
int mmhip_clip_to_yuv420(mmhip_invocation *inv, const void *src_rgba, int64_t src_row_stride, int64_t src_frame_stride, int width,
                         int height, int first_row, int last_row, int num_frames, int matrix, int range, void *dst,
                         int64_t dst_frame_stride, void *stream);
/* width * height + 2 * cw * ch: the bytes of one frame's payload (needs no GPU).  -1 for a size below 1 x 1. */
int64_t mmhip_yuv420_frame_bytes(int width, int height);
/* The stream header of a YUV4MPEG2 file of such frames (needs no GPU):
   "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" (or FULL), NUL-terminated, into buf of `cap` bytes.
   A frame in the file is "FRAME\n" followed by one frame's payload.  Returns the header's length without the NUL, or -1. */
int mmhip_y4m_header(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range);
/* The other direction: planar Y'CbCr 4:2:0 frames as an input drawable.  Converts num_frames payloads in device memory
   -- the layout mmhip_clip_to_yuv420 writes and a YUV4MPEG2 file holds -- to the packed words of a drawable, on the GPU
   (k_yuv420_to_rgba_clip, one launch).  Device to device, asynchronous on `stream` (0: the invocation's).  This statement
   is the specification: tests/yuv_input_reference.py restates it, mathmap_amd/csrc/mm_yuv.h holds it.
     - Source: every frame is one contiguous payload: the Y plane, width * height bytes with rows `width` apart, then Cb,
       then Cr, each cw * ch bytes with cw = (width + 1) >> 1 and ch = (height + 1) >> 1, rows cw apart.  Frames are
       src_frame_stride bytes apart, at least mmhip_yuv420_frame_bytes.  An odd last column or row has its own chroma
       sample.
     - Destination: packed frames of width * height uint32 words, rows `width` words apart, frames dst_frame_stride bytes
       apart: a multiple of 4 and at least 4 * width * height.  With dst_frame_stride = 4 * width * height this is what
       mmhip_set_image_sequence_device takes.  Nothing is written between or behind frames.
     - Arithmetic: all int32, every >> an arithmetic shift of a signed value (a floor division).  Per pixel, with Cb' and
       Cr' the chroma the pixel sees (below),
         y = Y - off, u = Cb' - 128, v = Cr' - 128
         R = clamp((ky * y + rcr * v + 2^15) >> 16, 0, 255)
         G = clamp((ky * y + gcb * u + gcr * v + 2^15) >> 16, 0, 255)
         B = clamp((ky * y + bcb * u + 2^15) >> 16, 0, 255)
       and the word is R << 24 | G << 16 | B << 8 | 255, the layout of mmhip_set_image_device; alpha is 255, as the RGB8
       upload forces it.  Out-of-range input (Y below 16 at limited range, chroma beyond 240) is legal and clamped:
       nothing is refused per sample.  No intermediate leaves int32 for any byte triple.
     - Coefficients: from the standard's constants Kr, Kb (0.299, 0.114 for bt601; 0.2126, 0.0722 for bt709) and Kg = 1 -
       Kr - Kb, the magnitude rounded as floor(|k| * 2^16 + 0.5) and the sign kept.  At limited range the luma scale is
       255/219, the chroma scale 255/224 and off 16; at full range both scales are 1 and off is 0.  ky = luma scale; rcr =
       2 (1 - Kr) * chroma scale; bcb = 2 (1 - Kb) * chroma scale; gcb = -2 (1 - Kb) Kb / Kg * chroma scale; gcr = -2 (1 -
       Kr) Kr / Kg * chroma scale:
         matrix, range    off   ky      rcr      gcb      gcr      bcb
         bt601 limited    16    76309   104597   -25675   -53279   132201
         bt601 full       0     65536   91881    -22553   -46802   116130
         bt709 limited    16    76309   117489   -13975   -34925   138438
         bt709 full       0     65536   103206   -12276   -30679   121609
       (235, 128, 128) at limited and (255, 128, 128) at full range give white, (16, 128, 128) and (0, 128, 128) black; at
       full range (v, 128, 128) gives v, v, v.
     - Chroma is sited at the centre of its 2 x 2 block (C420jpeg, what the writer emits).  chroma is
         MMHIP_YUV_CHROMA_REPLICATE: pixel (x, y) takes sample (x >> 1, y >> 1);
         MMHIP_YUV_CHROMA_BILINEAR (the Python and CLI default): cx = x >> 1, nx = clamp(cx + (x & 1 ? 1 : -1), 0, cw - 1),
           cy and ny likewise from y and ch, and
           C' = (9 * C[cy][cx] + 3 * C[cy][nx] + 3 * C[ny][cx] + C[ny][nx] + 8) >> 4
           for Cb and Cr alike: an 8-bit value before the matrix is applied.
     - The kernel has a path of aligned wide accesses (width a multiple of 8, src_yuv and src_frame_stride multiples of 8,
       dst_rgba32 and dst_frame_stride multiples of 16) and a path of byte loads and 4-byte stores for everything else;
       the launcher chooses, the words are the same.  mmhip_clip_from_yuv420_launches counts the launches of each.
       MMHIP_YUV_IN_STORES=cached|nt (read per call, default cached) selects plain or non-temporal stores.  Timed as
       yuv420_to_rgba_clip (mmhip_drain_native_kernel_ms).
   Errors, by name: width or height below 1; num_frames below 1 or above 65 535; an unknown matrix, range or chroma mode;
   null pointers; a src_frame_stride below one frame; a dst_frame_stride that is not a multiple of 4 or below one frame; a
   destination frame of more than 4 GiB (offsets inside a frame are 32-bit). */
enum { MMHIP_YUV_CHROMA_BILINEAR = 0, MMHIP_YUV_CHROMA_REPLICATE = 1 };
enum { MMHIP_YUV_IN_PATH_ALIGNED = 0, MMHIP_YUV_IN_PATH_BYTES = 1 };
int mmhip_clip_from_yuv420(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames,
                           int matrix, int range, int chroma, void *dst_rgba32, int64_t dst_frame_stride, void *stream);
/* The converter's launches of this invocation on path MMHIP_YUV_IN_PATH_ALIGNED or MMHIP_YUV_IN_PATH_BYTES; -1 for
   another path. */
long mmhip_clip_from_yuv420_launches(mmhip_invocation *inv, int path);
/* Binds num_frames host payloads, frame_stride bytes apart (at least mmhip_yuv420_frame_bytes), as the sequence of image
   user value `index`: allocates the owned sequence as mmhip_set_image_sequence_host does (the same refusals of sizes,
   the same release of the upload it replaces), uploads the payloads as they are -- 1.5 bytes per pixel -- in groups
   through a device staging buffer of at most MMHIP_CLIP_YUV_IN_BYTES (default 256 MiB, read per call, always at least one
   frame), converts every group with one mmhip_clip_from_yuv420 launch and binds the result through
   mmhip_set_image_sequence_device.  Everything documented for sequences holds unchanged: in(xy, n), white for a missing
   frame, native filters and mmhip_set_native_input_frame.  Synchronous.  mmhip_clip_yuv_input_groups returns the groups
   of the last such call of the invocation. */
int mmhip_set_image_sequence_yuv420_host(mmhip_invocation *inv, int index, const uint8_t *yuv, int64_t frame_stride, int width,
                                         int height, int num_frames, int matrix, int range, int chroma);
int mmhip_clip_yuv_input_groups(mmhip_invocation *inv);
/* Reads the stream header of a YUV4MPEG2 file from the first `len` bytes of buf (needs no GPU).  Accepted tags: the magic
   word YUV4MPEG2, W and H, an optional F (default 25:1), A (ignored), I of p or ?, no C tag or C420jpeg, C420mpeg2,
   C420paldv or C420 -- all read as 8-bit 4:2:0 with centre siting: the co-sited variants (C420mpeg2, C420paldv) are read
   as centre-sited, a shift of a quarter pixel that is not corrected -- XCOLORRANGE=FULL or LIMITED, and other X tags
   (ignored).  *range receives MMHIP_YUV_FULL or MMHIP_YUV_LIMITED, or -1 where the header does not state it;
   *header_len the bytes up to and including the newline.  A frame follows as a line beginning with FRAME (parameters
   may follow the word) and one payload.  Refuses by name: another magic word; a missing or non-positive W or H; an
   interlaced stream; every other colour space (C422, C444, C420p10, Cmono, ...); a malformed F; a header without a
   newline within len.  Returns 0, or -1. */
int mmhip_y4m_parse_header(const char *buf, int len, int *width, int *height, int *fps_num, int *fps_den, int *range, int *header_len);
/* A clip as 10-bit planar Y'CbCr 4:2:0 (yuv420p10): converts num_frames float frames in device memory -- what every clip
   entry point above but the supersampled one leaves with floatmap = 1 -- to the payloads of a YUV4MPEG2 file of colour
   space C420p10, on the GPU (k_float_to_yuv420p10_clip, one launch), so that nothing the clip computed in float is lost to
   an 8-bit store first.  Asynchronous on `stream` (0: the invocation's).  This statement is the specification:
   tests/yuv10_reference.py restates it, mathmap_amd/csrc/mm_yuv.h holds it.
     - Source: frames of width x height float4 RGBA pixels (16 bytes per pixel), of which the rows [first_row, last_row)
       are converted.  src points at row first_row of frame 0; rows are src_row_stride bytes apart (at least 16 * width),
       frames src_frame_stride; src and both strides are multiples of 4.  Alpha is not read.
     - Per channel: c = CLAMP01(v) as the pixel store clamps (NaN and -0 give 0, +inf gives 1), then
         q = (int)rintf(c * 65535.0f)
       one float32 product rounded to nearest with ties to even: 0 .. 65535.  NumPy:
       np.rint(np.float32(c) * np.float32(65535)).astype(np.int32).
     - Arithmetic: from here on all int32, every >> an arithmetic shift of a signed value (a floor division).  Per pixel
         Y = ((yr * R + yg * G + yb * B + 2^19) >> 20) + off
       Per chroma sample (cx, cy), with Rs, Gs, Bs the sums of q over the four pixels (min(2 cx + i, width - 1), min(2 cy +
       j, height - 1)), i, j in {0, 1} -- an odd last column or row is replicated; chroma is sited at the centre of the
       block (the siting of C420jpeg) --
         Cb = clamp(((cbr * Rs + cbg * Gs + cbb * Bs + 2^20) >> 21) + 512, 0, 1023)
         Cr likewise with crr, crg, crb.
     - Coefficients: from the standard's constants Kr, Kb (0.299, 0.114 for bt601; 0.2126, 0.0722 for bt709) and Kg = 1 -
       Kr - Kb.  The luma row is k = (Kr, Kg, Kb); the Cb row (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)), the Cr row (1 - Kr, -Kg,
       -Kb) / (2 (1 - Kr)).  With the channel in 0 .. 65535 the luma excursion E is 876 (limited, off 64) or 1023 (full, off
       0) and the chroma excursion 896 or 1023.  A luma coefficient is floor(k * E / 65535 * 2^20 + 0.5), a chroma
       coefficient sign(k) * floor(|k| * E / 65535 * 2^19 + 0.5).  The green coefficient of every row is not rounded by
       itself: it makes the luma row sum to the rounded coefficient of k = 1 and each chroma row sum to 0 (white is Y 940
       or 1023 exactly, black 64 or 0, every grey has chroma 512):
         matrix, range    off   yr, yg, yb            cbr, cbg, cbb          crr, crg, crb
         bt601 limited    64    4191, 8227, 1598      -1210, -2374, 3584     3584, -3001, -583
         bt601 full       0     4894, 9608, 1866      -1381, -2711, 4092     4092, -3427, -665
         bt709 limited    64    2980, 10024, 1012     -821, -2763, 3584      3584, -3255, -329
         bt709 full       0     3480, 11706, 1182     -938, -3154, 4092      4092, -3717, -375
       The largest luma intermediate is 1 073 201 168 and the chroma intermediates lie in [-1 072 676 880, 1 073 725 456]:
       inside int32 with room to spare (at scale 2^20 the full-range chroma would end 32 736 below 2^31, hence 2^19).  Limited-range chroma stays in 64 ..
       960 and full-range chroma in 1 .. 1023 without the clamp: pure blue and pure red, 1023.5 in the real formula,
       give 1023 (4092 is rounded down), so the clamp is a guard no colour reaches.
     - Destination: every frame is one contiguous payload of 16-bit little-endian samples with the value in the low 10
       bits: the Y plane, width * height samples with rows `width` samples apart, then Cb, then Cr, each cw * ch samples
       with cw = (width + 1) >> 1 and ch = (height + 1) >> 1, rows cw samples apart: 2 * (width * height + 2 * cw * ch)
       bytes (mmhip_yuv420p10_frame_bytes).  Frames are dst_frame_stride bytes apart, even and at least the payload.  dst
       (even) is the base of frame 0's whole-frame layout, for a row band too.
     - A band writes the Y rows [first_row, last_row) and the chroma rows [first_row / 2, (last_row + 1) / 2) and nothing
       else: no byte between frames, of other rows or behind the planes.  first_row must be even and last_row even or
       equal to height; under these two rules bands converted separately give the bytes of a whole-frame call.
     - The kernel has a path of aligned wide accesses (width a multiple of 8; src, both source strides, dst and
       dst_frame_stride multiples of 16) and a path of per-pixel loads and 2-byte stores for everything else; the launcher
       chooses, the bytes are the same.  mmhip_clip_float_to_yuv420p10_launches counts the launches of each.
       MMHIP_YUV10_COLUMNS=4|8 (read per call, default 4) sets the columns a work-item of the aligned path converts,
       MMHIP_YUV10_LOADS=cached|nt (read per call, default cached) plain or non-temporal loads.  Timed as yuv420p10_clip
       (mmhip_drain_native_kernel_ms).
   Errors, by name, in the wording of mmhip_clip_to_yuv420 where the condition is the same: width or height below 1;
   num_frames below 1 or above 65 535; an unknown matrix or range; rows that are not rows of the frame; an odd first_row;
   an odd last_row that is not height; null pointers; a src_row_stride below one row; a source pointer or stride that is
   not a multiple of 4; a dst_frame_stride below one frame; an odd dst or dst_frame_stride; a Y plane or a source band of
   more than 4 GiB (offsets inside a frame are 32-bit). */
enum { MMHIP_YUV10_PATH_ALIGNED = 0, MMHIP_YUV10_PATH_BYTES = 1 };
int mmhip_clip_float_to_yuv420p10(mmhip_invocation *inv, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width,
                                  int height, int first_row, int last_row, int num_frames, int matrix, int range, void *dst,
                                  int64_t dst_frame_stride, void *stream);
/* 2 * (width * height + 2 * cw * ch): the bytes of one frame's 10-bit payload (needs no GPU).  -1 for a size below 1 x 1. */
int64_t mmhip_yuv420p10_frame_bytes(int width, int height);
/* The stream header of a YUV4MPEG2 file of such frames (needs no GPU): the line of mmhip_y4m_header with C420p10 in
   place of C420jpeg, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n" (or FULL).  A frame in the file is
   "FRAME\n" followed by one frame's payload.  Returns the header's length without the NUL, or -1. */
int mmhip_y4m_header_p10(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range);
/* The converter's launches of this invocation on path MMHIP_YUV10_PATH_ALIGNED or MMHIP_YUV10_PATH_BYTES; -1 for another
   path. */
long mmhip_clip_float_to_yuv420p10_launches(mmhip_invocation *inv, int path);
/* The other direction at 10 bits: planar Y'CbCr 4:2:0 frames of 16-bit samples as a float32 input drawable.  Converts
   num_frames payloads in device memory -- the layout mmhip_clip_float_to_yuv420p10 writes and a YUV4MPEG2 file of colour
   space C420p10 holds -- to the float4 texels a filter compiled with deep_inputs = 1 binds, on the GPU
   (k_yuv420p10_to_float_clip, one launch), so that no 8-bit step stands between a 10-bit stream and the filter.  Device to
   device, asynchronous on `stream` (0: the invocation's).  This statement is the specification:
   tests/yuv10_input_reference.py restates it, mathmap_amd/csrc/mm_yuv.h holds it.
     - Source: every frame is one contiguous payload of 16-bit little-endian samples: the Y plane, width * height samples
       with rows `width` samples apart, then Cb, then Cr, each cw * ch samples with cw = (width + 1) >> 1 and ch = (height
       + 1) >> 1, rows cw samples apart: mmhip_yuv420p10_frame_bytes in all.  src_yuv and src_frame_stride are even; the
       stride is at least one payload.  A sample s is read as min(s, 1023): nothing is refused per sample.
     - Chroma the pixel sees, at scale 16, an exact integer that is not rounded back to 10 bits (centre siting, as in
       mmhip_clip_from_yuv420).  chroma is
         MMHIP_YUV_CHROMA_REPLICATE: S = 16 * C[y >> 1][x >> 1];
         MMHIP_YUV_CHROMA_BILINEAR (the Python and CLI default): cx = x >> 1, nx = clamp(cx + (x & 1 ? 1 : -1), 0, cw - 1),
           cy and ny likewise from y and ch, and
           S = 9 * C[cy][cx] + 3 * C[cy][nx] + 3 * C[ny][cx] + C[ny][nx]
       for Cb and Cr alike; u = S_cb - 8192, v = S_cr - 8192.
     - To float: yf = (float)(Y - off), uf = (float)u, vf = (float)v, all three exact; off and the luma excursion E are 64
       and 876 (limited) or 0 and 1023 (full).  L = yf / (float)E is one IEEE float32 division; every * and + below is one
       float32 operation rounded to nearest, none contracted to an fma (the device uses __fdiv_rn, __fmul_rn, __fadd_rn):
         R = L + vf * rcr
         G = (L + uf * gcb) + vf * gcr
         B = L + uf * bcb
         A = 1.0f
       There is no clamp: below-black and super-white samples become values below 0 and above 1, as a deep drawable
       allows; a filter that wants them gone clamps them itself.
     - Coefficients: from the standard's constants Kr, Kb (0.299, 0.114 for bt601; 0.2126, 0.0722 for bt709), Kg = 1 - Kr -
       Kb and the chroma excursion Ec = 896 (limited) or 1023 (full), per 1/16 chroma unit: rcr = 2 (1 - Kr) / (16 Ec); bcb
       = 2 (1 - Kb) / (16 Ec); gcb = -2 (1 - Kb) Kb / (Kg * 16 Ec); gcr = -2 (1 - Kr) Kr / (Kg * 16 Ec); each the float32
       nearest to the exact rational value:
         matrix, range    off   E      rcr               gcb                gcr                bcb
         bt601 limited    64    876    0x1.9a2f66p-14f   -0x1.92bce0p-16f   -0x1.a1df2ap-15f   0x1.0337e2p-13f
         bt601 full       0     1023   0x1.67434ap-14f   -0x1.60bd72p-16f   -0x1.6dfec6p-15f   0x1.c61350p-14f
         bt709 limited    64    876    0x1.ccbdd2p-14f   -0x1.b67222p-17f   -0x1.11eb6ap-15f   0x1.0f72a2p-13f
         bt709 full       0     1023   0x1.938afap-14f   -0x1.8003e0p-17f   -0x1.dfd3eep-16f   0x1.db7f7ap-14f
       With chroma 512 R == G == B for every Y; Y = off gives 0.0f and Y = off + E 1.0f exactly; at limited range Y = 0
       gives -0.07305936f and Y = 1023 1.0947489f.  A grey frame that goes on through mmhip_clip_float_to_yuv420p10 in
       the same mode returns every legal Y code unchanged.
     - Destination: frames of width * height float4 texels, rows 16 * width bytes apart, frames dst_frame_stride bytes
       apart; dst_float4 and dst_frame_stride are multiples of 16 and the stride is at least 16 * width * height.  With
       dst_frame_stride = 16 * width * height this is what mmhip_set_image_sequence_float_device takes.  Nothing is
       written between or behind frames.
     - The kernel has a path of aligned wide accesses (width a multiple of 8, src_yuv and src_frame_stride multiples of
       16; the destination is aligned by the rule above) and a path of 2-byte loads and per-pixel stores for everything
       else; the launcher chooses, the floats are the same.  mmhip_clip_from_yuv420p10_launches counts the launches of
       each.  MMHIP_YUV10_IN_COLUMNS=2|4|8 (read per call, default 2) sets the columns a work-item of the aligned path
       converts, MMHIP_YUV10_IN_STORES=cached|nt (read per call, default cached) plain or non-temporal stores; the
       defaults are the fastest of the six measured.  Timed as yuv420p10_to_float_clip
       (mmhip_drain_native_kernel_ms).
   Errors, by name, in the wording of mmhip_clip_from_yuv420 where the condition is the same: width or height below 1;
   num_frames below 1 or above 65 535; an unknown matrix, range or chroma mode; null pointers; an odd src_yuv or
   src_frame_stride; a src_frame_stride below one payload; a dst_float4 or dst_frame_stride that is not a multiple of 16;
   a dst_frame_stride below one frame; a destination frame of more than 4 GiB (offsets inside a frame are 32-bit). */
enum { MMHIP_YUV10_IN_PATH_ALIGNED = 0, MMHIP_YUV10_IN_PATH_SAMPLES = 1 };
int mmhip_clip_from_yuv420p10(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames,
                              int matrix, int range, int chroma, void *dst_float4, int64_t dst_frame_stride, void *stream);
/* The converter's launches of this invocation on path MMHIP_YUV10_IN_PATH_ALIGNED or MMHIP_YUV10_IN_PATH_SAMPLES; -1 for
   another path. */
long mmhip_clip_from_yuv420p10_launches(mmhip_invocation *inv, int path);
/* Binds num_frames host payloads of 16-bit samples (in the host's byte order), frame_stride bytes apart (even, at least
   mmhip_yuv420p10_frame_bytes), as the float32 sequence of image user value `index`, as
   mmhip_set_image_sequence_float_host binds float frames: the same refusals, before anything is allocated (sizes, a null
   pointer, a filter compiled without deep_inputs), then the converter's own.  The payloads go up as they are -- 3 bytes
   per pixel instead of 16 -- in groups through a device staging buffer of at most MMHIP_CLIP_YUV_IN_BYTES (default 256
   MiB, read per call, always at least one frame); every group takes one mmhip_clip_from_yuv420p10 launch into the owned
   sequence, which is bound as a deep image; the upload it replaces is released.  Synchronous.
   mmhip_clip_yuv10_input_groups returns the groups of the last such call of the invocation. */
int mmhip_set_image_sequence_yuv420p10_host(mmhip_invocation *inv, int index, const uint16_t *yuv, int64_t frame_stride, int width,
                                            int height, int num_frames, int matrix, int range, int chroma);
int mmhip_clip_yuv10_input_groups(mmhip_invocation *inv);
/* mmhip_y4m_parse_header for streams of either depth: accepts everything that function accepts, with *bits = 8, and the
   colour space C420p10 with *bits = 10 (a frame's payload is then mmhip_yuv420p10_frame_bytes of little-endian 16-bit
   samples).  Every other refusal is that function's.  Needs no GPU.  Returns 0, or -1. */
int mmhip_y4m_parse_stream_header(const char *buf, int len, int *width, int *height, int *fps_num, int *fps_den, int *range, int *bits,
                                  int *header_len);
/* Convenience: whole frame to a host RGBA8 buffer (width*height*4 bytes); synchronous. */
int mmhip_render_host(mmhip_invocation *inv, int frame, float t, uint8_t *out_rgba);
int mmhip_sync(mmhip_invocation *inv);
/* Average device time (ms) of the last pixel-kernel launch as measured with HIP
   events on the launch stream; requires mmhip_enable_timing(inv, 1). */
int mmhip_enable_timing(mmhip_invocation *inv, int on);
double mmhip_last_kernel_ms(mmhip_invocation *inv);
/* Durations of the pixel kernel of all timed launches since the last drain (oldest first, waits
   for the last one): lets a caller queue many launches without a synchronisation per launch. */
int mmhip_drain_kernel_ms(mmhip_invocation *inv, double *out_ms, int cap);
/* Durations (ms) of the kernels native filters launched themselves (gaussian_blur's scan kernels) since the last
   drain, in launch order; names receives a 64-byte label per entry.  Requires mmhip_enable_timing(inv, 1). */
int mmhip_drain_native_kernel_ms(mmhip_invocation *inv, char *names, double *out_ms, int cap);
/* Launches of this invocation whose pixels a native filter wrote itself -- a filter like
   examples/Blur/Gaussian Blur.mm, whose pixel is the blurred map sampled at the pixel centre: the
   blur's last kernel packs the output (new_template.c.in:279-293) and the pixel kernel is skipped. */
long mmhip_direct_native_launches(mmhip_invocation *inv);
/* Launches of this invocation whose pixels gaussian_blur's tolerance chain wrote (gauss_mode MMHIP_GAUSS_TOLERANCE and the
   conditions stated at mmhip_options.gauss_mode). */
long mmhip_tolerance_blur_launches(mmhip_invocation *inv);
/* Launches of the prologue kernel (mm_prologue) that mmhip_render made for this invocation, one per launch, the nested
   renders of mmhip_render_supersampled included; a render that found its frame constants standing adds nothing. */
long mmhip_prologue_launches(mmhip_invocation *inv);
/* Native filter calls of this invocation's single-frame renders that were answered from the memo: same arguments on
   unchanged inputs, so the map of the earlier call was kept and no native kernel ran for the call. */
long mmhip_native_memo_hits(mmhip_invocation *inv);

/* device memory helpers for callers without their own allocator */
void *mmhip_device_alloc(size_t bytes);
void mmhip_device_free(void *p);
int mmhip_copy_to_host(void *dst_host, const void *src_device, size_t bytes);
int mmhip_copy_to_device(void *dst_device, const void *src_host, size_t bytes);
int mmhip_device_count(void);
/* One process per GPU: selects the device (ordinal among the visible ones) the calling thread's later
   mmhip_* calls use -- invocations, their streams, modules and buffers live on the device that is
   current when they are created.  Returns 0, or -1 with mmhip_last_error(). */
int mmhip_set_device(int ordinal);

/* Chroma siting for the four 4:2:0 converters above.  Everything stated there places a chroma sample at the centre of its
   2 x 2 luma block (MMHIP_YUV_SITING_CENTER: JPEG siting, C420jpeg), and every function above keeps doing exactly that.
   H.264, HEVC and AV1 streams under BT.709 and BT.601 carry chroma co-sited with the even luma column of the block and
   centred between its two rows (MMHIP_YUV_SITING_LEFT: MPEG-2 or "left" siting, C420mpeg2): it is what a decoder writes
   into a Y4M pipe and what an encoder assumes on the way in.  Read with the wrong siting, the colour planes shift
   against luma by a quarter of a luma pixel in each direction of the conversion.  The _sited functions below are the
   functions above with an `int siting` argument after `range` (out) or `chroma` (in): the same parameters, layouts,
   paths, counters, timing labels and environment variables; the same refusals in the same order under their own names
   (clip_to_yuv420_sited: ...), and one more, made after the matrix, range and chroma checks and before anything is
   allocated, launched or bound: "siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not N".  With
   MMHIP_YUV_SITING_CENTER each is the function above: the same kernel instantiation, the same bytes.  This statement is
   the specification of MMHIP_YUV_SITING_LEFT: tests/yuv_sited_reference.py restates it, mathmap_amd/csrc/mm_yuv.h holds
   it.  Top-left siting (BT.2020) and the siting of C420paldv are not modelled.
     - Out, left siting (mmhip_clip_to_yuv420_sited, mmhip_clip_float_to_yuv420p10_sited).  Luma is unchanged.  Chroma
       sample (cx, cy) is computed from six pixels: the columns 2 cx - 1, 2 cx, 2 cx + 1 with the weights 1, 2, 1 -- a
       column below 0 is column 0, a column at or above width is width - 1 -- and the rows 2 cy and 2 cy + 1 with weight 1
       each -- a row at or above height is height - 1.  Rs, Gs, Bs are the weighted sums of the bytes at 8 bits, of the
       quantised channels q (mmhip_clip_float_to_yuv420p10) at 10 bits; the weights sum to 8.  With the mode's
       coefficients as they stand in the tables above, every / a floor division,
         8 bits:   Cb = clamp(((cbr * Rs + cbg * Gs + cbb * Bs + 2^18) >> 19) + 128, 0, 255)
         10 bits:  Cb = clamp(floor((cbr * Rs + cbg * Gs + cbb * Bs + 2^21) / 2^22) + 512, 0, 1023)
       and Cr likewise.  At 8 bits the sums are at most 2040 and a row's absolute coefficients sum to at most 65 536: the
       intermediate stays below 2^27, all int32.  At 10 bits the sums reach 524 280; a row's coefficients have both signs,
       so k . sums and each of its partial sums lies within +-4092 * 524 280 = +-2 145 353 760 and the intermediate with
       its rounding term in [-2 143 256 608, 2 147 450 912]: twice the centre form's, the upper end 32 736 below 2^31.
       An int32 would hold that by a margin the centre form changes its scale to avoid, so this one expression is
       computed in int64, where nothing depends on the margin; the shift leaves -511 .. 511, a sample in 1 .. 1023 before
       the clamp (pure blue and pure red at full range give 1023).  A chroma row of coefficients sums to 0: grey
       gives 128 and 512 exactly, as at centre siting.  On a frame whose columns 2 cx - 1, 2 cx, 2 cx + 1 are equal the
       sample is the centre-sited one (sums of 8 against 4, one more bit of shift).
     - In, left siting, chroma MMHIP_YUV_CHROMA_BILINEAR (mmhip_clip_from_yuv420_sited, mmhip_clip_from_yuv420p10_sited).
       Vertically unchanged: with cy = y >> 1 and ny = clamp(cy + (y & 1 ? 1 : -1), 0, ch - 1), the column sum at chroma
       column i is col(i) = 3 * C[cy][i] + C[ny][i] (at 10 bits of samples read as min(s, 1023)).  Horizontally an even
       pixel column lies on its chroma column and an odd one half way to the next: with cx = x >> 1 and r = min(cx + 1,
       cw - 1),
                   even x                       odd x
         8 bits:   C' = (4 * col(cx) + 8) >> 4  C' = (2 * col(cx) + 2 * col(r) + 8) >> 4
         10 bits:  S = 4 * col(cx)              S = 2 * col(cx) + 2 * col(r)
       the weights sum to 16; the 10-bit S stays at scale 16 and is not rounded.  Everything after the chroma the pixel
       sees is unchanged: the matrix and the clamps at 8 bits, u = S_cb - 8192, v = S_cr - 8192 and the explicit float32
       operations at 10.  A work-item reads its own and the right chroma column only, one column fewer than centre
       siting.
     - chroma MMHIP_YUV_CHROMA_REPLICATE ignores the siting: either value is accepted and gives the bytes of centre.
     - The host setters upload and group as the functions above and convert every group with the _sited converter; what
       the converter refuses is refused under its _sited name before anything is allocated or bound. */
enum { MMHIP_YUV_SITING_CENTER = 0, MMHIP_YUV_SITING_LEFT = 1 };
int mmhip_clip_to_yuv420_sited(mmhip_invocation *inv, const void *src_rgba, int64_t src_row_stride, int64_t src_frame_stride, int width,
                               int height, int first_row, int last_row, int num_frames, int matrix, int range, int siting, void *dst,
                               int64_t dst_frame_stride, void *stream);
int mmhip_clip_float_to_yuv420p10_sited(mmhip_invocation *inv, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width,
                                        int height, int first_row, int last_row, int num_frames, int matrix, int range, int siting, void *dst,
                                        int64_t dst_frame_stride, void *stream);
int mmhip_clip_from_yuv420_sited(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames,
                                 int matrix, int range, int chroma, int siting, void *dst_rgba32, int64_t dst_frame_stride, void *stream);
int mmhip_clip_from_yuv420p10_sited(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames,
                                    int matrix, int range, int chroma, int siting, void *dst_float4, int64_t dst_frame_stride, void *stream);
int mmhip_set_image_sequence_yuv420_host_sited(mmhip_invocation *inv, int index, const uint8_t *yuv, int64_t frame_stride, int width,
                                               int height, int num_frames, int matrix, int range, int chroma, int siting);
int mmhip_set_image_sequence_yuv420p10_host_sited(mmhip_invocation *inv, int index, const uint16_t *yuv, int64_t frame_stride, int width,
                                                  int height, int num_frames, int matrix, int range, int chroma, int siting);
/* The stream header of a YUV4MPEG2 file for frames of `bits` 8 or 10 with a siting (needs no GPU).  With
   MMHIP_YUV_SITING_CENTER the line of mmhip_y4m_header (bits 8) or mmhip_y4m_header_p10 (bits 10), byte for byte.  With
   MMHIP_YUV_SITING_LEFT at 8 bits the same line with C420mpeg2 in place of C420jpeg:
   "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n" (or FULL).  At 10 bits the C420p10 line unchanged:
   Y4M has no tag for the siting of a 10-bit stream, so tell the encoder.  Refuses, by name, bits that are neither, an
   unknown siting, and what mmhip_y4m_header refuses.  Returns the header's length without the NUL, or -1. */
int mmhip_y4m_header_sited(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range, int bits, int siting);
/* The chroma siting a stream header states (needs no GPU): *siting receives MMHIP_YUV_SITING_LEFT for C420mpeg2 and
   MMHIP_YUV_SITING_CENTER for no C tag, C420, C420jpeg, C420paldv and C420p10.  C420paldv (co-sited columns, Cb and Cr on
   alternating rows) is not modelled and is read as centre, as mmhip_y4m_parse_header reads it; C420p10 cannot say.
   Refuses what mmhip_y4m_parse_stream_header refuses, in its words, under the name y4m_stream_siting.  Returns 0, or -1. */
int mmhip_y4m_stream_siting(const char *buf, int len, int *siting);

#ifdef __cplusplus
}
#endif
#endif
