// IR -> HIP C++ kernel string.  The MI355X counterpart of the reference's
// backends/cc.c (which fills new_template.c.in and shells out to gcc).
#pragma once
#include <string>
#include <vector>

#include "ir.h"

namespace mm {

struct KernelOptions {
    int intersample = 1;      // bilinear input fetch (CLI flag -i)
    int supersampling = 0;
    int edge_x = 0, edge_y = 0;
    int pixel_inc = 1;        // stride of the image sources the bilinear fetch interpolates over (the GIMP preview's fast source)
    int deep_inputs = 0;      // 1: the generic fetch knows float32 drawables (MM_IMG_DEEP; #define MM_DEEP_INPUTS 1)
    int tile_w = 0;           // pixels per workgroup row (0: chosen from the body, auto_tile_w); tile_h = 256 / tile_w
    int unroll = 0;           // pixels evaluated back to back per work-item step; 0 = choose (hipgen.cpp auto_unroll)
    bool hoist = true;        // evaluate frame-constant code once per frame in a prologue kernel
    bool fast_math_exact = true;   // use f32 paths only where bit-identical to the double path
    // The shutter variant of the module (fused motion blur): mm_prologue_clip and mm_rows_clip as the clip variant has
    // them, and mm_pixels_shutter in place of the pixel kernel -- single-pixel shape, the pixel body in a loop over a
    // pixel's sub-samples, their sum in registers.  Generated a second time from the code `source` was generated from
    // (the row slice is taken as that run left it); filters without native calls only.
    bool shutter = false;
    // The sampled variant (fused grid supersampling, with or without a shutter): like the shutter variant, with
    // mm_pixels_sampled in its place -- the loop runs over the K * sx * sy sub-samples of a pixel, x and y of a sub-sample
    // come from per-offset coordinate tables that this variant's own mm_prologue_clip writes.  Filters without native
    // calls and without a per-row slice only (the slice's values follow y: such filters take the maps path).
    bool sampled = false;
    // The refine variant (adaptive anti-aliasing, mmhip_render_clip_adaptive): the sampled variant's mm_prologue_clip,
    // text unchanged, and mm_pixels_refine in place of mm_pixels_sampled -- the same loop over a pixel's sub-samples, the
    // pixel taken from a per-frame list (mm_refine) instead of the tile order.  Set together with `sampled`.
    bool refine = false;
    bool variant() const { return shutter || sampled; }      // a second generation from the code of the main text
};

// One native-filter (or render) call found in the frame-constant code.
struct NativeCall {
    std::string func;             // "native_filter_gaussian_blur", "RENDER", ...
    std::vector<Ty> arg_types;
    int record_offset = 0;        // byte offset of its record in the frame-constant buffer
    bool in_loop = false;         // a call site inside a `while': its calls are numbered as they happen and recorded in
                                  // the dynamic entries (below); its own record stays unexecuted
    bool dynamic = false;         // one of the MM_NATIVE_DYN_CALLS entries behind the call sites: the n-th call made
                                  // from any in-loop site of this frame (the record's `index' names the site)
};

enum { MM_NATIVE_REC_BYTES = 320, MM_NATIVE_ARG_BYTES = 32, MM_NATIVE_MAX_ARGS = 9, MM_NATIVE_DYN_CALLS = 16 };

struct KernelSource {
    std::string source;           // full translation unit (prelude + 2 kernels)
    std::string prologue_name, pixel_name;
    int xy_bytes = 0;             // size of the frame-constant buffer
    bool has_prologue = false;
    std::vector<NativeCall> natives;      // the call sites, then -- if a site sits in a loop -- MM_NATIVE_DYN_CALLS dynamic entries
    int native_sites = 0;         // number of call sites among `natives'
    int native_ctr_offset = -1;   // int[4] in the frame-constant buffer: calls made so far (program order), dynamic
                                  // entries taken, "more in-loop calls than dynamic entries" flag
    int tile_w = 16, tile_h = 16;
    int unroll = 1;               // MM_UNROLL of the pixel kernel; the launch's rows per work-item is a multiple
    bool prologue_uses_time = true;   // frame-constant code reads t or frame: re-run it for every frame
    bool single_pixel = false;    // kernel renders exactly one pixel per work-item: launch with ppt = 1
    bool pair_mode = false;       // the pixel loop evaluates two vertically adjacent rows in lockstep (unroll 2)
    bool pair_exit = false;       // ... with exit-driven loops: the kernels for which a peeled first trip is kept
    int xcd_order = 2;            // MM_XCD_ORDER: workgroup -> tile order of the pixel kernel
    int row_values = 0;           // > 0: kernel `mm_rows` fills that many per-row values (mm_args.rowtab) before the pixel kernel
    std::string rows_name;
    int direct_native = -1;       // index into natives: the pixel is that result sampled at (x, y) and nothing else
    std::string key;              // cache key (hash of source)
    // Compile with -fwrapv.  apply_edge_behaviour (builtins.c:40-119) negates and mirrors coordinates in ints (`-x % width`,
    // `(height - 1) - y`), and a coordinate that is NaN, infinite or beyond +-2^31 px arrives there as INT_MIN (mm_f2i): the
    // reference's x86 ints wrap (-INT_MIN is INT_MIN, INT_MIN % n is negative: the pixel stays outside), while signed overflow
    // is undefined for the compiler, which turned INT_MIN % 13 into a texel inside the image.  Set for REFLECT and ROTATE edges,
    // the only code with such arithmetic; every other kernel is compiled as before.
    bool wrapping_ints = false;
    // The clip variant of the module (mm_prologue_clip, mm_rows_clip, mm_pixels_clip): `source` with these spans
    // replaced, in order -- the kernels' heads; every body is the same text (clip_kernel_source)
    struct Splice { size_t begin, end; std::string text; };
    std::vector<Splice> clip_splices;
};

// `functions_of`: the code whose `functions` (filter_$name bodies) `code` may call; null = its own
KernelSource generate_hip(FilterCode &code, const KernelOptions &opt, FilterCode *functions_of = nullptr);
// Is peeling first loop trips (peel_first_trips, passes.h) switched on?  MMHIP_PAIR_PEEL=1: on (default off).  The caller peels a specialised
// filter's code, generates, and compiles again without peeling unless the kernel came out in exit-driven pair mode.
bool pair_peel_enabled();
// the clip variant's text and its cache key, built from `ks.source` on demand
void clip_kernel_source(const KernelSource &ks, std::string *source, std::string *key);
const char *clip_prelude();
const char *clip_prelude_natives();   // ... of a filter with native-filter calls: mm_clip.images_stride
const char *shutter_prelude();        // mm_shutter, behind clip_prelude() in the shutter variant (KernelOptions::shutter)
const char *sampled_prelude();        // mm_sampled, behind clip_prelude() in the sampled variant (KernelOptions::sampled)
const char *refine_prelude();         // mm_refine, in front of mm_pixels_refine in the refine variant (KernelOptions::refine)
const char *device_prelude();
const char *device_noise_prelude();   // mm_noise_device.h
const char *device_fastmath_prelude();   // mm_fastmath.h + tables
const char *noise_table_text();        // nullptr when the libnoise table was not available at build time

}  // namespace mm
