// Internal definitions shared by runtime.cpp, runtime_clip.cpp and abi_backend.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mmhip.h"
#include "front.h"
#include "hipgen.h"
#include "mm_host_abi.h"
#include "native_filters.h"

namespace mm { void load_ir_json(Module &mod, FilterCode &code, const char *json); }   // ir_json.cpp

// One module of a filter: its text (with key and kernel names), its code object, and the loaded module with its kernels
// (f_rows: where the text has a per-row slice, ks.row_values > 0, and the owner launches it).
struct ModuleVariant {
    mm::KernelSource ks;
    std::vector<char> code_object;
    hipModule_t mod = nullptr;
    hipFunction_t f_pro = nullptr, f_rows = nullptr, f_pix = nullptr;
    bool loaded = false;
};
enum { VARIANT_CLIP, VARIANT_SHUTTER, VARIANT_SAMPLED, VARIANT_REFINE, VARIANT_COUNT };

// The kernels that render closure image #k of a filter into a float map (FilterCode::closure_renders[k]):
// same user values and images as the owning filter, own code object.
using mmhip_closure_kernel = ModuleVariant;

struct mmhip_filter {
    std::vector<mmhip_closure_kernel> closures;
    mm::Module module;
    std::unique_ptr<mm::FilterCode> code;
    mm::KernelOptions kopt;
    mm::KernelSource ks;
    std::string ir_json;        // after the passes: what the kernels were generated from
    std::string ir_json_raw;    // straight out of lowering (or the importer), before any pass: what the
                                // oracle prints, so that the passes are tested differentially
    std::vector<char> code_object;
    hipModule_t mod = nullptr;
    hipFunction_t f_pro = nullptr, f_pix = nullptr;
    hipFunction_t f_rows = nullptr;           // the per-row slice's kernel (KernelSource::row_values > 0)
    bool loaded = false;
    double jit_seconds = 0;
    // the variants of the module that clip rendering launches, each built when it is first asked for (runtime.cpp
    // variant_source, jit_variant).  clip (mmhip_render_clip): made from the main text, for every filter.  shutter
    // (mmhip_render_clip_shutter_fused, KernelOptions::shutter): generated from `code`; filters without native calls or
    // closure images.  sampled (mmhip_render_clip_sampled_fused, KernelOptions::sampled): the same under its own key;
    // filters that have no per-row slice either.  refine (mmhip_render_clip_adaptive, KernelOptions::refine): the fifth
    // module, under its own key; the filters that have a sampled variant.
    ModuleVariant variants[VARIANT_COUNT];
    // user-value specialisation (specialize.cpp): kernels with the scalar user values baked in,
    // keyed by the value bytes; owned by this filter
    std::string source;
    mmhip_options opts{};
    bool specialize = false;
    std::map<std::string, mmhip_filter *> spec_cache;
    struct SpecUse { int count = 0; int frame = 0; float t = 0.0f; };
    std::map<std::string, SpecUse> spec_uses; // frames seen per value set that has no variant yet
    int spec_min_uses = 1;                    // build the variant on this many-th render with one value set
    // a filter that only compiles with its scalar user values baked in (recursion whose depth
    // they control): no generic code/kernels, every render goes through spec_cache
};

// A device allocation the owner frees by going out of scope.
struct DeviceBuffer {
    void *p = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
        if (this != &o) { reset(); p = std::exchange(o.p, nullptr); bytes = std::exchange(o.bytes, 0); }
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T = void> T *get() const { return (T *)p; }
    explicit operator bool() const { return p != nullptr; }
    static hipError_t no_wait() { return hipSuccess; }
    // At least `need` bytes: a larger request frees the old buffer once `wait()` has returned hipSuccess (what may still
    // read it is the caller's to say) and allocates a new one, zero-filled with `zero`.  A failed allocation leaves the
    // buffer empty, so that the next call allocates again.
    template <class Wait = hipError_t (*)()> hipError_t grow(size_t need, Wait wait = no_wait, bool zero = false) {
        if (need <= bytes) return hipSuccess;
        if (p) {
            const hipError_t e = wait();
            if (e != hipSuccess) return e;
            reset();
        }
        hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = need;
        if (zero && (e = hipMemset(p, 0, need)) != hipSuccess) reset();
        return e;
    }
};

// What a launch's kernels keep besides the tables and the output: frame constants, per-column / per-row coordinates,
// per-row values (mm_rows: [value][row]).
struct LaunchBuffers { DeviceBuffer xy, xtab, ytab, rowtab; };

// Host memory the device reads directly (page-locked), freed by its owner.
struct PinnedBuffer {
    void *p = nullptr;
    size_t bytes = 0;
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    ~PinnedBuffer() { if (p) (void)hipHostFree(p); }
    hipError_t grow(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        const hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = need;
        return hipSuccess;
    }
};

// What the batches of a clip render keep (mmhip_render_clip): one frame-constant slot and one row table per frame of a
// batch (a single one of each where the prologue does not read t or frame), and the {t, frame} table of the call.  The
// table goes up from page-locked memory; two of them alternate, so that a call need not wait for the one before it.
struct ClipBuffers {
    DeviceBuffer xy, rowtab;
    struct Table {
        PinnedBuffer host;
        DeviceBuffer dev;
        hipEvent_t uploaded = nullptr;      // recorded behind the table's copy: the host side may be rewritten after it
        bool pending = false;
        ~Table() { if (uploaded) (void)hipEventDestroy(uploaded); }
    } table[2];
    unsigned next_table = 0;
};

// What the native batches of a clip render keep (clip_native_batch in runtime_clip.cpp), apart from the single-frame path's
// maps and workspace: checkpoints and intermediates of one call site's jobs, the maps of a batch's blurs, and the tables
// the kernels index by frame and by job (every frame's image table, then the job tables), which go up from page-locked memory.
struct ClipNativeBuffers {
    DeviceBuffer work, maps, tables;
    PinnedBuffer host;
    hipEvent_t uploaded = nullptr;          // recorded behind the tables' copy: `host' may be rewritten after it
    bool uploaded_pending = false;
    ~ClipNativeBuffers() { if (uploaded) (void)hipEventDestroy(uploaded); }
};

// Native call entry k (KernelSource::natives[k]): its float4 map and what is remembered about it.
struct NativeEntry {
    DeviceBuffer map;
    int w = 0, h = 0;                          // the render size the map was allocated for
    // Every recomputation of the map gets a new generation (the reference gives every native result a new image id,
    // cache.c:65-68); the memo records the generations of the native maps among its image arguments, so a consumer is
    // recomputed when its producer was.
    unsigned long long gen = 0;
    mm::HNativeRec memo{};                     // args of the call that produced the map
    int memo_frame = 0, seen_frame = 0;        // ... and the frame of a sequence it read (MMHIP_NATIVE_FRAME_CURRENT; else NO_FRAME_KEY)
    unsigned long long memo_gen = 0;
    std::vector<unsigned long long> memo_deps;
    mm::HNativeRec seen{};                     // last argument set whose map was asked for (direct output: materialised on its second use)
    unsigned long long seen_gen = ~0ULL;
    std::pair<int, int> rows{0, 0};            // rows of the map that are valid
};

// The invocation's own stream: its first member, so that it is destroyed after every buffer.
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream &) = delete;
    ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

struct mmhip_invocation {
    ~mmhip_invocation();
    OwnedStream stream;
    mmhip_filter *f = nullptr;
    int img_w = 0, img_h = 0, render_w = 0, render_h = 0;
    std::vector<mm::HUserval> uv;
    std::vector<mm::HImageDesc> images;
    std::vector<int> image_slot_of_uv;     // userval index -> image table slot (or -1)
    std::vector<float> curves;             // [n_curves][1024] (userval.h:37, userval.c:282-311)
    std::vector<uint32_t> gradients;       // [n_gradients][1024] packed 0xRRGGBBAA
    DeviceBuffer d_uv, d_images, d_curves, d_gradients;
    int native_slot_base = 0;
    bool tables_dirty = true;
    std::vector<DeviceBuffer> owned;       // device buffers we allocated for input images
    std::vector<NativeEntry> natives;
    unsigned long long native_gen_counter = 0;
    // closure images rendered for native filters: float map, the sub-launch's own buffers, the maps of the native
    // filters the closure's own code calls
    struct ClosureState {
        DeviceBuffer map;
        int w = 0, h = 0;
        LaunchBuffers launch;
        int native_slot_base = 0;
        std::vector<DeviceBuffer> native_results;
    };
    std::vector<ClosureState> closure_state;
    DeviceBuffer ss_lines;                 // the two slices of a supersampled render (own allocation: native filters
                                           // reallocate `ws` underneath a nested render)
    int native_row_margin = -1;                     // mmhip_set_native_row_margin
    int native_input_frame = 0;                     // mmhip_set_native_input_frame
    long direct_native_launches = 0;                // mmhip_direct_native_launches
    long tolerance_blur_launches = 0;               // mmhip_tolerance_blur_launches
    long prologue_launches = 0;                     // mmhip_prologue_launches
    long native_memo_hits = 0;                      // mmhip_native_memo_hits
    // the prologue kernel is skipped while nothing it reads has changed (mmhip_render)
    mm::HArgs pro_args{};
    const mmhip_filter *pro_filter = nullptr;
    void *pro_stream = nullptr;
    unsigned long long pro_generation = 0, table_generation = 1;
    unsigned long long input_generation = 1;
    LaunchBuffers launch;                  // of the main kernels (mmhip_render)
    ClipBuffers clip;                      // of the clip kernels (mmhip_render_clip)
    long clip_batched_launches = 0;        // mmhip_clip_batched_launches
    long clip_prologue_frames = 0;         // mmhip_clip_prologue_frames
    ClipNativeBuffers clip_native;         // of the native batches of a clip render
    long clip_native_batches = 0;          // mmhip_clip_native_batches
    long clip_native_blurs = 0;            // mmhip_clip_native_blurs
    long clip_native_direct_frames = 0;    // mmhip_clip_native_direct_frames
    DeviceBuffer clip_ss;                  // the slices of a batch of supersampled frames (mmhip_render_clip_supersampled):
                                           // every frame's long slice, then every frame's short slice
    long clip_supersampled_batches = 0;    // mmhip_clip_supersampled_batches
    DeviceBuffer clip_shutter;             // the sub-sample float maps of a batch of motion-blurred frames
                                           // (mmhip_render_clip_shutter), and behind them the carry map where one is needed
    long clip_shutter_batches = 0;         // mmhip_clip_shutter_batches
    long clip_shutter_fused_batches = 0;   // mmhip_clip_shutter_fused_batches
    long clip_sampled_batches = 0;         // mmhip_clip_sampled_batches
    long clip_sampled_fused_batches = 0;   // mmhip_clip_sampled_fused_batches
    DeviceBuffer clip_sampled;             // of a fused grid-supersampled batch: the grid's offsets (16 floats), then the
                                           // per-offset x tables and y tables (mm_sampled, hipgen.cpp sampled_prelude)
    // adaptive anti-aliasing (mmhip_render_clip_adaptive): a batch's base maps and, behind them, its lists of the pixels to
    // refine; the refined-pixel counts of every frame of the last call, and the stream that call ran on
    DeviceBuffer clip_adaptive, clip_adaptive_counts;
    int clip_adaptive_frames = 0;
    hipStream_t clip_adaptive_stream = nullptr;
    long clip_adaptive_batches = 0;        // mmhip_clip_adaptive_batches
    // filtered clips (mmhip_render_clip_filtered): the tap blocks of both axes by edge class, as built on the host and
    // as the combine reads them; the maps are the shutter's temporary
    std::vector<unsigned> clip_filter_host;
    DeviceBuffer clip_filter_taps;
    long clip_filtered_batches = 0;        // mmhip_clip_filtered_batches
    // YUV 4:2:0 input (mmhip_clip_from_yuv420, mmhip_set_image_sequence_yuv420_host): the converter's launches by the
    // path the launcher took (aligned, byte), and the upload groups of the last host call
    long clip_yuv_input_launches[2] = {0, 0};
    int clip_yuv_input_groups = 0;
    // 10-bit YUV 4:2:0 output from float frames (mmhip_clip_float_to_yuv420p10): the converter's launches by path
    long clip_yuv10_launches[2] = {0, 0};
    // 10-bit YUV 4:2:0 input to float frames (mmhip_clip_from_yuv420p10, mmhip_set_image_sequence_yuv420p10_host): the
    // converter's launches by path, and the upload groups of the last host call
    long clip_yuv10_input_launches[2] = {0, 0};
    int clip_yuv10_input_groups = 0;
    uint32_t edge_color_x = 0, edge_color_y = 0;
    float sampling_offset_x = 0.f, sampling_offset_y = 0.f;
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // the pair of the most recent launch (aliases into ev_pool)
    bool ev_valid = false;
    // one event pair per timed launch, so a caller can queue many launches and read all durations
    // afterwards without a synchronisation per launch (mmhip_drain_kernel_ms)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    mm::NativeWorkspace ws;
};


extern thread_local std::string g_mmhip_err;   // message behind mmhip_last_error()

// Two-step construction from already lowered IR (used by the reference-ABI importer):
// create, fill f->module (filters, main) and f->code, then finalize (passes + codegen).
mmhip_filter *mmhip_filter_new_empty();
bool mmhip_filter_finalize(mmhip_filter *f, const mm::KernelOptions &ko, std::string *err);
// false (and mmhip_last_error) for options mmhip_compile* refuses
bool mmhip_check_options(const mmhip_options *opts);

// Unbinds every image-table entry that refers to `data` (a device buffer about to be freed).
void mmhip_unbind_image(mmhip_invocation *inv, const void *data);

// ---- what clip rendering (runtime_clip.cpp) uses of the single-frame path: defined, and described, in runtime.cpp ----
inline int fail(const std::string &msg) { g_mmhip_err = msg; return -1; }

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The launch geometry of a pixel kernel over `num_rows` rows of a `region_w`-wide region: the one place both launch
// sites (mmhip_render, render_closure) and mmhip_filter_launch_geometry take it from.
struct LaunchGeometry {
    int tiles_x = 0, tiles_y = 0;
    long wg1 = 0;                 // workgroups at one row per work-item: what the rows-per-item choice is made from
    long nwg = 0;                 // workgroups of the launch
    int ppt = 1;                  // rows per work-item (mm_args.ppt)
    uint32_t tiles_magic = 0;     // mm_args.tiles_magic
};
LaunchGeometry clip_launch_geometry(const mm::KernelSource &ks, int region_w, int num_rows, int frames);
// ... of a kernel of the single-pixel shape with the tiles of `ks` (mm_pixels_shutter): one row per work-item
LaunchGeometry single_pixel_launch_geometry(const mm::KernelSource &ks, int region_w, int num_rows);
// max_frames is the smaller of the two caps it is made of: grid rows (gridDim.y, MMHIP_CLIP_MAX_FRAMES) and work-items
struct ClipPlan { long grid_x = 0; int max_frames = 0; int max_grid_rows = 0; long max_rows_by_items = 0; };
ClipPlan clip_plan(const LaunchGeometry &g);

mmhip_filter *active_filter(mmhip_invocation *inv, int frame = 0, float t = 0.0f);
mm::HArgs render_args(const mmhip_invocation *inv, int frame, float t, int region_x, int region_y, int region_w, int region_h,
                      int first_row, int last_row, void *out_device, int row_stride, int bpp, int floatmap);
int upload_tables(mmhip_invocation *inv, hipStream_t s);
int grow_launch_buffers(LaunchBuffers &b, const mm::KernelSource &ks, int region_w, int num_rows, bool rows, hipStream_t s);
bool clamp_rows(int region_y, int region_h, int *first_row, int *last_row);
int timed_pixel_launch(mmhip_invocation *inv, hipFunction_t f_pix, unsigned grid_x, unsigned grid_y, void **params, hipStream_t s);

struct RecordedCall { size_t k; mm::HNativeRec rec; const std::string *func; };
int recorded_calls(const mm::KernelSource &ks, const char *host, std::vector<RecordedCall> *calls);
enum { NO_FRAME_KEY = INT32_MIN };
int view_sequence_args(const mmhip_invocation *inv, int frame, const std::string &func, const mm::HNativeRec &rec,
                       std::vector<mm::HImageDesc> &images_k, int *frame_key);
mm::HImageDesc floatmap_desc(const void *data, int w, int h);
void set_native_env(mmhip_invocation *inv, const mmhip_filter *f, bool gauss_tolerance);
bool direct_output_wanted(const mmhip_filter *f, const mm::HArgs &a);
int read_coordinate_tables(const mm::HArgs &a, hipStream_t s, std::vector<float> *xt, std::vector<float> *yt);
bool samples_own_pixels(const mm::HArgs &a, const std::vector<float> &xt, const std::vector<float> &yt);

// The invocation's sampling offsets for the length of a scope: put back on every way out.
struct SamplingOffsetGuard {
    mmhip_invocation *inv;
    float ox, oy;
    explicit SamplingOffsetGuard(mmhip_invocation *i) : inv(i), ox(i->sampling_offset_x), oy(i->sampling_offset_y) {}
    ~SamplingOffsetGuard() { inv->sampling_offset_x = ox; inv->sampling_offset_y = oy; }
    void set(float v) { inv->sampling_offset_x = inv->sampling_offset_y = v; }
    void set(float x, float y) { inv->sampling_offset_x = x; inv->sampling_offset_y = y; }
};
