// Clip rendering: the frames of an animation in batched launches (mmhip_render_clip), supersampled
// (mmhip_render_clip_supersampled) and motion-blurred (mmhip_render_clip_shutter through sub-sample maps,
// mmhip_render_clip_shutter_fused in the pixel kernel's registers), grid-supersampled (mmhip_render_clip_sampled,
// mmhip_render_clip_sampled_fused: the same two ways) and adaptively so (mmhip_render_clip_adaptive), on top of the
// single-frame path of runtime.cpp.  Every entry point checks its arguments into a ClipTarget (clip_target), the paths
// hand that to each other (render_clip_to, render_clip_maps), and whatever launches a variant's kernels over batches of
// frames does so through clip_call_begin and clip_call_run.
// (The exported functions have C linkage from include/mmhip.h.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "clip_kernels.h"
#include "mm_clip_filter.h"
#include "mm_sample_grid.h"
#include "mm_shutter_combine.h"
#include "mm_yuv.h"
#include "runtime_internal.h"

using namespace mm;

// A byte budget from the environment: a positive count, or the default.
static size_t env_bytes(const char *name, size_t fallback) {
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : fallback;
}

// The argument checks every entry point makes, under the name of the one that was called.
static int check_clip_args(const char *who, int num_frames, const int *frames, const float *ts, int bpp, int region_w, int region_h) {
    if (num_frames < 1) return fail(std::string(who) + ": num_frames must be at least 1");
    if (!frames || !ts) return fail(std::string(who) + ": frames and ts must be arrays of num_frames entries");
    if (bpp < 1 || bpp > 4) return fail("output_bpp must be 1..4");
    if (region_w <= 0 || region_h <= 0) return fail("empty region");
    return 0;
}

// what one frame's band occupies: the next frame must begin behind it (the invocation is looked at for float maps only)
static int check_frame_stride(const char *who, const mmhip_invocation *inv, int64_t frame_stride, int num_rows, int region_w, int row_stride, int bpp, int floatmap) {
    const int64_t band = floatmap ? (int64_t)num_rows * 16 * inv->render_w
                                  : (int64_t)(num_rows - 1) * row_stride + (int64_t)region_w * bpp;
    if (frame_stride < band)
        return fail(std::string(who) + ": frame_stride " + std::to_string(frame_stride) + " is smaller than one frame's band (" +
                    std::to_string(band) + " bytes)");
    return 0;
}

long mmhip_clip_batched_launches(mmhip_invocation *inv) { return inv->clip_batched_launches; }
long mmhip_clip_prologue_frames(mmhip_invocation *inv) { return inv->clip_prologue_frames; }
long mmhip_clip_native_batches(mmhip_invocation *inv) { return inv->clip_native_batches; }
long mmhip_clip_native_blurs(mmhip_invocation *inv) { return inv->clip_native_blurs; }
long mmhip_clip_native_direct_frames(mmhip_invocation *inv) { return inv->clip_native_direct_frames; }

// mm_clip of the clip kernels (hipgen.cpp clip_prelude; images_stride is `pad' in the text of filters without native calls)
struct HClipFrame { float t; int frame; };
struct HClip { const HClipFrame *frames; long long frame_stride; int xy_stride; int rowtab_stride; int nwg; int images_stride; };
static_assert(sizeof(HClip) == 32, "mm_clip layout");

// ---- clip batches of filters whose native calls are gaussian_blur ----
// May the native calls of `f' run as batches over the frames of a clip?  Every call site a gaussian_blur outside loops,
// no closure images, the exact chain with one segment per line, whole maps.
static bool clip_native_eligible(const mmhip_filter *f, int native_row_margin) {
    if (f->ks.natives.empty() || f->ks.native_sites != (int)f->ks.natives.size() || !f->closures.empty()) return false;
    for (const NativeCall &nc : f->ks.natives)
        if (nc.func != "native_filter_gaussian_blur") return false;
    const char *seg = getenv("MMHIP_GAUSS_SEGMENTS");
    return f->opts.gauss_mode == MMHIP_GAUSS_EXACT && !(seg && *seg) && native_row_margin < 0;
}

// Frames per batch: the clip plan's, at most 65 535 jobs per launch, and what MMHIP_CLIP_NATIVE_BYTES (read once,
// default 8 GiB) holds of one frame's checkpoints, intermediate and result of every call site.  Below 2 the clip is
// rendered frame by frame.
struct ClipNativePlan { bool eligible = false; int per_batch = 0; size_t bytes_per_frame = 0; };
static ClipNativePlan clip_native_plan(const mmhip_filter *f, int native_row_margin, const ClipPlan &plan, int render_w, int render_h) {
    static const size_t budget = env_bytes("MMHIP_CLIP_NATIVE_BYTES", (size_t)8 << 30);
    ClipNativePlan p;
    p.eligible = clip_native_eligible(f, native_row_margin);
    if (!p.eligible || render_w < 1 || render_h < 1) return p;
    size_t ck = 0, map = 0;
    gaussian_blur_batch_job_bytes(render_w, render_h, &ck, &map);
    p.bytes_per_frame = (size_t)f->ks.native_sites * (ck + 2 * map);
    const size_t by_bytes = budget / p.bytes_per_frame;
    const int per = (int)std::min<size_t>(std::min(plan.max_frames, 65535), by_bytes);
    p.per_batch = per < 2 ? 0 : per;
    return p;
}

int mmhip_filter_clip_native_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int render_h, int frames, int64_t *out) {
    if (frames < 1) return fail("clip native plan: num_frames must be at least 1");
    if (region_w < 1 || num_rows < 1 || render_w < 1 || render_h < 1) return fail("clip native plan: empty region");
    const ClipPlan cp = clip_plan(clip_launch_geometry(f->ks, region_w, num_rows, frames));
    const ClipNativePlan p = clip_native_plan(f, -1, cp, render_w, render_h);
    const int64_t v[MMHIP_CLIP_NATIVE_PLAN_FIELDS] = {p.eligible, p.per_batch, p.per_batch ? (frames + p.per_batch - 1) / p.per_batch : 0,
                                                      (int64_t)p.bytes_per_frame};
    memcpy(out, v, sizeof v);
    return 0;
}

// Where a clip call lands: the region, its rows clamped to the region, the output and its layout, the stream.  Every
// entry point fills one (clip_target) and the paths hand it to each other.
struct ClipTarget {
    int region_x, region_y, region_w, region_h;
    int first_row, last_row, num_rows;
    void *out;
    int row_stride;
    int64_t frame_stride;
    int bpp, floatmap;
    hipStream_t s;
    // the same rows of the same region as float maps at `maps`, a frame every `stride` bytes: what a path renders its
    // intermediates to
    ClipTarget as_floatmaps(void *maps, int64_t stride) const {
        ClipTarget t = *this;
        t.out = maps;
        t.frame_stride = stride;
        t.floatmap = 1;
        return t;
    }
    // frame b0 of the call as the first one
    ClipTarget from_frame(int b0) const {
        ClipTarget t = *this;
        t.out = (char *)out + (int64_t)b0 * frame_stride;
        return t;
    }
    // where a combine kernel stores the frames (clip_kernels.h)
    ClipStore store() const { return ClipStore{out, row_stride, frame_stride, bpp, floatmap}; }
};

// Fills `tg` from an entry point's arguments and makes the checks all of them share, under the name of the one that was
// called: -1 refused, 0 nothing to render (no row of the region is asked for), 1 filled.  `span`: the shutter's, 0 for a
// call without one.  `in_render_width`: the paths that go through float maps of the render width want the region inside
// it.  The invocation is not looked at before a check needs it.
static int clip_target(const char *who, const mmhip_invocation *inv, float span, int num_frames, const int *frames, const float *ts,
                       int region_x, int region_y, int region_w, int region_h, int first_row, int last_row, void *out_device, int row_stride,
                       int64_t frame_stride, int bpp, int floatmap, void *stream, bool in_render_width, ClipTarget *tg) {
    if (!std::isfinite(span)) return fail(std::string(who) + ": span must be finite");
    if (check_clip_args(who, num_frames, frames, ts, bpp, region_w, region_h) != 0) return -1;
    if (!clamp_rows(region_y, region_h, &first_row, &last_row)) return 0;
    const int num_rows = last_row - first_row;
    if (check_frame_stride(who, inv, frame_stride, num_rows, region_w, row_stride, bpp, floatmap) != 0) return -1;
    if (in_render_width && region_w > inv->render_w) return fail(std::string(who) + ": the region is wider than the render width");
    *tg = ClipTarget{region_x, region_y, region_w, region_h, first_row, last_row, num_rows, out_device, row_stride, frame_stride,
                     bpp, floatmap, stream ? (hipStream_t)stream : (hipStream_t)inv->stream};
    return 1;
}

// What one batched clip call hands its batches: the module that is launched and how, as the caller's plan has it, and
// what clip_call_begin makes of that.
struct ClipCall {
    mmhip_invocation *inv;
    mmhip_filter *f;
    const ModuleVariant *v;    // the variant whose kernels are launched
    hipStream_t s;
    LaunchGeometry geo;
    long grid_x;               // of the pixel launch
    bool per_frame;            // else one frame-constant slot and one row table for all frames
    size_t xy_stride, rowtab_stride;      // of one slot: bytes, floats
    const int *frames;
    const float *ts;
    // from clip_call_begin
    HArgs a{};                 // out: the first frame of the call
    HClip c{};                 // frames: the call's table
    char *xy = nullptr;
    bool rows = false;
    ClipBuffers::Table *tab = nullptr;
    // native batches: the records of the shared slot (read with the first batch) and whether the launch samples a
    // native map at every pixel's own centre (decided once per call)
    std::vector<char> records;
    int direct_ok = -1;
};

// Frame constants (and the per-row slice) of frames [b0, b0 + n): one grid row per frame -- or, where they do not depend on
// t and frame (!per_frame), frame 0's once for the whole call.  Returns the frames they were launched for, or -1.
// (f_pro, f_rows: mm_prologue_clip and, where the filter has a per-row slice, mm_rows_clip of the module that is launched)
static int launch_clip_prologue(hipFunction_t f_pro, hipFunction_t f_rows, const HArgs &a, bool per_frame, int b0, int n, void **params, hipStream_t s) {
    const unsigned pro_x = (unsigned)((std::max(a.region_width, a.num_rows) + 255) / 256), rows_x = (unsigned)((a.num_rows + 255) / 256);
    const unsigned pro_frames = per_frame ? (unsigned)n : b0 == 0 ? 1u : 0u;
    if (pro_frames) {
        HIP_TRY(hipModuleLaunchKernel(f_pro, pro_x, pro_frames, 1, 256, 1, 1, 0, s, params, nullptr));
        if (f_rows) HIP_TRY(hipModuleLaunchKernel(f_rows, rows_x, pro_frames, 1, 256, 1, 1, 0, s, params, nullptr));
    }
    return (int)pro_frames;
}

// The {t, frame} table of a whole call, `entries` of them: the next of the invocation's two tables, free to be written
// at its host side when this returns; send_clip_table then copies it up.  The caller's arrays are free after that.
static int next_clip_table(mmhip_invocation *inv, size_t entries, hipStream_t s, ClipBuffers::Table **out) {
    ClipBuffers::Table &tab = inv->clip.table[inv->clip.next_table++ & 1];
    if (tab.pending) HIP_TRY(hipEventSynchronize(tab.uploaded));
    tab.pending = false;
    const size_t tab_bytes = entries * sizeof(HClipFrame);
    HIP_TRY(tab.host.grow(tab_bytes));
    HIP_TRY(tab.dev.grow(tab_bytes, [s] { return hipStreamSynchronize(s); }));
    if (!tab.uploaded) HIP_TRY(hipEventCreateWithFlags(&tab.uploaded, hipEventDisableTiming));
    *out = &tab;
    return 0;
}

static int send_clip_table(ClipBuffers::Table &tab, size_t entries, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(tab.dev.get(), tab.host.p, entries * sizeof(HClipFrame), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(tab.uploaded, s));
    tab.pending = true;
    return 0;
}

// Frames [b0, b0 + n) of a clip of a filter whose native calls are all gaussian_blur: one prologue launch, one read-back
// of all its records, every distinct blur of a call site in one gaussian_blur_batch, one pixel launch over per-frame
// image tables -- or none, where the blurs pack the frames' bytes themselves.  A batch with a call the batched blur does
// not take (a FIR deviation, an input of another size, ...) is rendered frame by frame before anything of it is written.
static int clip_native_batch(ClipCall &cc, int b0, int n) {
    mmhip_invocation *inv = cc.inv;
    mmhip_filter *f = cc.f;
    hipStream_t s = cc.s;
    const KernelSource &ks = f->ks;
    HArgs a = cc.a;
    HClip c = cc.c;
    char *xy = cc.xy;
    a.out = (char *)cc.a.out + (int64_t)b0 * cc.c.frame_stride;
    c.frames = cc.c.frames + b0;
    c.images_stride = 0;          // the prologue (and the per-row slice) of every frame reads the invocation's table
    void *params[] = {&a, &xy, &c};
    const int pro_frames = launch_clip_prologue(cc.v->f_pro, cc.rows ? cc.v->f_rows : nullptr, a, cc.per_frame, b0, n, params, s);
    if (pro_frames < 0) return -1;
    if (pro_frames) {
        cc.records.resize(cc.xy_stride * pro_frames);
        HIP_TRY(hipMemcpyAsync(cc.records.data(), xy, cc.records.size(), hipMemcpyDeviceToHost, s));
    }
    std::vector<float> xt, yt;
    const bool ask_direct = cc.direct_ok < 0 && direct_output_wanted(f, a) && (cc.c.frame_stride & 3) == 0;
    if (ask_direct && read_coordinate_tables(a, s, &xt, &yt) != 0) return -1;
    HIP_TRY(hipStreamSynchronize(s));      // (and with it for the batch before this one: its buffers are free)
    if (cc.direct_ok < 0) cc.direct_ok = ask_direct && samples_own_pixels(a, xt, yt) ? 1 : 0;
    auto frame_by_frame = [&]() -> int {
        for (int i = b0; i < b0 + n; ++i)
            if (mmhip_render(inv, cc.frames[i], cc.ts[i], a.region_x, a.region_y, a.region_width, a.region_height, a.first_row,
                             a.first_row + a.num_rows, (char *)cc.a.out + (int64_t)i * cc.c.frame_stride, a.row_stride, a.output_bpp, a.floatmap,
                             cc.s) != 0)
                return -1;
        return 0;
    };

    // Computations: in call order, frames share one where the call site, the record and the computations behind its
    // native-map arguments are equal -- what the memo does for a loop of single renders.
    // (view: the image table with the sequence argument's frame in place, MMHIP_NATIVE_FRAME_CURRENT; else empty)
    struct Comp { size_t k; HNativeRec rec; int frame; std::vector<HImageDesc> view; float *map = nullptr; };
    const int sites = ks.native_sites, base = inv->native_slot_base;
    std::vector<Comp> comps;
    std::vector<int> of_frame((size_t)n * sites, -1);      // [frame][site] -> computation
    std::map<std::string, int> known;
    std::vector<char> is_dep;
    std::vector<RecordedCall> calls;
    for (int i = 0; i < n; ++i) {
        if (recorded_calls(ks, cc.records.data() + (cc.per_frame ? (size_t)i * cc.xy_stride : 0), &calls) != 0) return -1;
        size_t last_k = 0;
        for (size_t q = 0; q < calls.size(); ++q) {
            const RecordedCall &call = calls[q];
            if (q > 0 && call.k <= last_k) return frame_by_frame();      // the sites are not in call order: not expected outside loops
            last_k = call.k;
            std::string key((const char *)&call.k, sizeof call.k);
            key.append((const char *)&call.rec, sizeof call.rec);
            for (int j = 0; j < call.rec.nargs && j < 4; ++j) {
                const HNativeArg &arg = call.rec.args[j];
                if (arg.kind != 2 || arg.img.idx < base || arg.img.idx >= base + sites) continue;
                const int dep = of_frame[(size_t)i * sites + (arg.img.idx - base)];
                key.append((const char *)&dep, sizeof dep);
                if (dep >= 0) is_dep[dep] = 1;
            }
            std::vector<HImageDesc> view;
            int frame_key = NO_FRAME_KEY;
            if (view_sequence_args(inv, cc.frames[b0 + i], *call.func, call.rec, view, &frame_key) != 0) return -1;
            key.append((const char *)&frame_key, sizeof frame_key);
            auto it = known.find(key);
            if (it == known.end()) {
                it = known.emplace(key, (int)comps.size()).first;
                comps.push_back(Comp{call.k, call.rec, i, std::move(view)});
                is_dep.push_back(0);
            }
            of_frame[(size_t)i * sites + call.k] = it->second;
        }
    }
    // direct output: the direct call's blur packs frame i's bytes -- every frame has a blur of its own there, and nothing else reads it
    bool direct = cc.direct_ok == 1 && ((uintptr_t)a.out & 3) == 0;
    if (direct) {
        std::vector<char> taken(comps.size(), 0);
        for (int i = 0; i < n && direct; ++i) {
            const int id = of_frame[(size_t)i * sites + ks.direct_native];
            direct = id >= 0 && !taken[id] && !is_dep[id];
            if (direct) taken[id] = 1;
        }
    }
    // buffers: checkpoints and intermediate per job of the largest site, a map per computation that is read
    size_t ck_bytes = 0, map_bytes = 0;
    gaussian_blur_batch_job_bytes(a.render_width, a.render_height, &ck_bytes, &map_bytes);
    std::vector<size_t> per_site(sites, 0);
    size_t kept = 0;
    for (const Comp &cp : comps) {
        ++per_site[cp.k];
        if (!(direct && (int)cp.k == ks.direct_native)) ++kept;
    }
    const size_t jobs_max = comps.empty() ? 0 : *std::max_element(per_site.begin(), per_site.end());
    const size_t images_n = inv->images.size();
    const size_t images_bytes = ((size_t)n * images_n * sizeof(HImageDesc) + 255) & ~(size_t)255;
    const size_t tables_bytes = images_bytes + gaussian_blur_batch_table_bytes(comps.size());
    ClipNativeBuffers &nb = inv->clip_native;
    auto idle = [] { return hipSuccess; };      // the stream has just been waited for
    HIP_TRY(nb.work.grow(jobs_max * (ck_bytes + map_bytes), idle));
    HIP_TRY(nb.maps.grow(kept * map_bytes, idle));
    HIP_TRY(nb.tables.grow(tables_bytes, idle));
    if (nb.uploaded_pending) HIP_TRY(hipEventSynchronize(nb.uploaded));
    nb.uploaded_pending = false;
    HIP_TRY(nb.host.grow(tables_bytes));
    {
        size_t m = 0;
        for (Comp &cp : comps)
            if (!(direct && (int)cp.k == ks.direct_native)) cp.map = (float *)(nb.maps.get<char>() + (m++) * map_bytes);
    }
    // every frame's image table: the invocation's, the native slots this frame's maps (the null image where a call did not execute)
    HImageDesc *tables = (HImageDesc *)nb.host.p;
    HImageDesc null_desc{};
    null_desc.kind = IMG_NULL;
    for (int i = 0; i < n; ++i) {
        HImageDesc *t = tables + (size_t)i * images_n;
        std::copy(inv->images.begin(), inv->images.end(), t);
        for (int k = 0; k < sites; ++k) {
            const int id = of_frame[(size_t)i * sites + k];
            t[base + k] = id >= 0 && comps[id].map ? floatmap_desc(comps[id].map, a.render_width, a.render_height) : null_desc;
        }
    }
    set_native_env(inv, f, false);
    // (a computation's own slot is still null in its frame's table while it is planned; a later one finds its map there)
    for (const Comp &cp : comps) {
        const int idx = cp.rec.args[0].img.idx;
        const HImageDesc *t = cp.view.empty() ? tables + (size_t)cp.frame * images_n : cp.view.data();
        const bool own_result = idx >= base && idx < base + sites && of_frame[(size_t)cp.frame * sites + (idx - base)] >= 0 && (size_t)(idx - base) < cp.k;
        const bool bound_input = idx >= 0 && idx < base;
        if (!(own_result || bound_input) ||
            !gaussian_blur_batchable(cp.rec, t, (int)images_n, a.render_width, a.render_height, inv->ws.env, nullptr, nullptr))
            return frame_by_frame();
    }
    // the job tables of every site, behind the image tables; one copy takes all of them up
    NativeDirectOut dout;
    dout.row_stride = a.row_stride;
    dout.first_row = a.first_row;
    dout.num_rows = a.num_rows;
    dout.region_x = a.region_x;
    dout.region_w = a.region_width;
    std::vector<std::vector<GaussClipGroup>> groups(sites);
    std::vector<GaussClipLaunch> launches(sites);
    size_t at = images_bytes;
    std::string err;
    for (int k = 0; k < sites; ++k) {
        std::vector<GaussClipJob> jobs;
        const bool packs = direct && k == ks.direct_native;
        for (size_t id = 0; id < comps.size(); ++id) {
            const Comp &cp = comps[id];
            if ((int)cp.k != k) continue;
            char *w = nb.work.get<char>() + jobs.size() * (ck_bytes + map_bytes);
            jobs.push_back(GaussClipJob{cp.rec, cp.view.empty() ? tables + (size_t)cp.frame * images_n : cp.view.data(), (int)images_n, (double *)w, (float *)(w + ck_bytes), cp.map,
                                        packs ? (unsigned char *)a.out + (int64_t)cp.frame * cc.c.frame_stride : nullptr});
        }
        launches[k].render_w = a.render_width;
        launches[k].render_h = a.render_height;
        launches[k].direct = packs ? &dout : nullptr;
        launches[k].write_map = !packs;
        if (jobs.empty()) continue;
        if (gaussian_blur_batch_tables(jobs, launches[k], inv->ws.env, (char *)nb.host.p + at, nb.tables.get<char>() + at, &groups[k], &err) != 0)
            return fail(err);
        at += gaussian_blur_batch_table_bytes(jobs.size());
    }
    if (!nb.uploaded) HIP_TRY(hipEventCreateWithFlags(&nb.uploaded, hipEventDisableTiming));
    HIP_TRY(hipMemcpyAsync(nb.tables.get(), nb.host.p, tables_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(nb.uploaded, s));
    nb.uploaded_pending = true;
    for (int k = 0; k < sites; ++k)
        if (!groups[k].empty() && gaussian_blur_batch_launch(groups[k], launches[k], inv->ws, s, &err) != 0) return fail(err);
    ++inv->clip_native_batches;
    inv->clip_native_blurs += (long)comps.size();
    if (direct) {
        inv->clip_native_direct_frames += n;
        return 0;
    }
    a.images = nb.tables.get<HImageDesc>();
    c.images_stride = (int)images_n;
    return timed_pixel_launch(inv, cc.v->f_pix, (unsigned)cc.grid_x, (unsigned)n, params, s);
}

// ---- the batched launch every path without native calls ends in ----
// What a batched call sets up before its first launch, for the kernels of `ks` (the text cc.v was made from) over the
// rows of `tg`: the invocation's tables, the launch arguments of frame frame0 at t0, room for `slots` frame-constant
// slots and row tables, and the next {t, frame} table with `entries` entries.  The caller writes the table's host side
// and sends it up (send_clip_table).
static int clip_call_begin(ClipCall &cc, const ClipTarget &tg, const KernelSource &ks, int frame0, float t0, size_t slots, size_t entries) {
    mmhip_invocation *inv = cc.inv;
    hipStream_t s = cc.s;
    if (upload_tables(inv, s) != 0) return -1;
    HArgs &a = cc.a;
    a = render_args(inv, frame0, t0, tg.region_x, tg.region_y, tg.region_w, tg.region_h, tg.first_row, tg.last_row, tg.out, tg.row_stride,
                    tg.bpp, tg.floatmap);
    cc.rows = ks.row_values > 0;
    // the coordinate tables are the single-frame path's, rewritten here: its prologue must run again
    if (grow_launch_buffers(inv->launch, ks, tg.region_w, tg.num_rows, false, s) != 0) return -1;
    inv->pro_filter = nullptr;
    auto wait = [s] { return hipStreamSynchronize(s); };
    HIP_TRY(inv->clip.xy.grow(cc.xy_stride * slots, wait, true));
    if (cc.rows) HIP_TRY(inv->clip.rowtab.grow(cc.rowtab_stride * slots * sizeof(float), wait));
    if (next_clip_table(inv, entries, s, &cc.tab) != 0) return -1;

    a.xtab = inv->launch.xtab.get<float>();
    a.ytab = inv->launch.ytab.get<float>();
    if (cc.rows) a.rowtab = inv->clip.rowtab.get<float>();
    a.ppt = cc.geo.ppt;
    a.tiles_magic = cc.geo.tiles_magic;
    cc.xy = inv->clip.xy.get<char>();
    cc.c = HClip{};
    cc.c.frames = cc.tab->dev.get<HClipFrame>();
    cc.c.frame_stride = tg.frame_stride;
    cc.c.xy_stride = cc.per_frame ? (int)cc.xy_stride : 0;
    cc.c.rowtab_stride = cc.per_frame ? (int)cc.rowtab_stride : 0;
    cc.c.nwg = (int)cc.geo.nwg;
    return 0;
}

// The launches of a call that clip_call_begin has set up: `num_frames` output frames, `per_batch` of them to a pixel
// launch, each with `per_frame_slots` entries of the table (1, or the sub-samples in time of a fused frame); the prologue
// (and the per-row slice) runs over a batch's slots.  params: &cc.a, &cc.xy, &cc.c and what the variant's kernels take
// behind them.  `launches` is the caller's counter of batches; without one the caller counts for itself, and the
// prologue's slots are not counted either.
static int clip_call_run(ClipCall &cc, int num_frames, int per_batch, int per_frame_slots, void **params, long *launches) {
    const ClipBuffers::Table &tab = *cc.tab;
    char *out = (char *)cc.a.out;
    for (int b0 = 0; b0 < num_frames; b0 += per_batch) {
        const int n = std::min(per_batch, num_frames - b0);
        cc.a.out = out + (int64_t)b0 * cc.c.frame_stride;
        cc.c.frames = tab.dev.get<HClipFrame>() + (size_t)b0 * per_frame_slots;
        const int pro_slots = launch_clip_prologue(cc.v->f_pro, cc.rows ? cc.v->f_rows : nullptr, cc.a, cc.per_frame, b0, n * per_frame_slots,
                                                   params, cc.s);
        if (pro_slots < 0) return -1;
        if (timed_pixel_launch(cc.inv, cc.v->f_pix, (unsigned)cc.grid_x, (unsigned)n, params, cc.s) != 0) return -1;
        if (launches) {
            cc.inv->clip_prologue_frames += pro_slots;
            ++*launches;
        }
    }
    return 0;
}

// The {t, frame} entries of `num_frames` frames with `samples` instants each (mm_shutter_sample_t; one instant is the
// frame's own t): slot i * samples + j is instant j of frame i.
static void fill_clip_table(HClipFrame *hf, int num_frames, const int *frames, const float *ts, int samples, float span) {
    for (int i = 0; i < num_frames; ++i)
        for (int j = 0; j < samples; ++j)
            hf[(size_t)i * samples + j] = HClipFrame{samples == 1 ? ts[i] : mm_shutter_sample_t(ts[i], span, j, samples), frames[i]};
}

// mmhip_render_clip behind its argument checks: what the other paths render their float maps with.
static int render_clip_to(mmhip_invocation *inv, const ClipTarget &tg, int num_frames, const int *frames, const float *ts) {
    mmhip_filter *f = active_filter(inv, frames[0], ts[0]);
    const LaunchGeometry geo = clip_launch_geometry(f->ks, tg.region_w, tg.num_rows, num_frames);
    const ClipPlan plan = clip_plan(geo);
    const bool natives = !f->ks.natives.empty();
    const ClipNativePlan nplan = natives ? clip_native_plan(f, inv->native_row_margin, plan, inv->render_w, inv->render_h) : ClipNativePlan();
    if ((natives && nplan.per_batch < 1) || !f->closures.empty() || plan.max_frames < 1) {
        // native filters run the host between prologue and pixels of every frame: frame by frame, the same result
        // (but for gaussian_blur calls the batches below take)
        for (int i = 0; i < num_frames; ++i)
            if (mmhip_render(inv, frames[i], ts[i], tg.region_x, tg.region_y, tg.region_w, tg.region_h, tg.first_row, tg.last_row,
                             (char *)tg.out + (int64_t)i * tg.frame_stride, tg.row_stride, tg.bpp, tg.floatmap, tg.s) != 0)
                return -1;
        return 0;
    }
    if (mmhip_filter_jit_clip(f, 1) < 0) return -1;
    const bool per_frame = f->ks.prologue_uses_time;
    const int per_batch = std::min(num_frames, natives ? nplan.per_batch : plan.max_frames);
    const size_t xy_stride = ((size_t)std::max(f->ks.xy_bytes, 256) + 255) / 256 * 256;
    const size_t rowtab_stride = (size_t)f->ks.row_values * tg.num_rows;
    const int slots = per_frame ? per_batch : 1;
    if (rowtab_stride * slots > (size_t)INT32_MAX || xy_stride * slots > (size_t)INT32_MAX)
        return fail("render_clip: the batch's row tables are too large; lower MMHIP_CLIP_MAX_FRAMES");
    ClipCall cc{inv, f, &f->variants[VARIANT_CLIP], tg.s, geo, plan.grid_x, per_frame, xy_stride, rowtab_stride, frames, ts};
    // the {t, frame} table of the whole call, copied now: the caller's arrays are free when this returns
    if (clip_call_begin(cc, tg, f->ks, frames[0], ts[0], (size_t)slots, (size_t)num_frames) != 0) return -1;
    fill_clip_table((HClipFrame *)cc.tab->host.p, num_frames, frames, ts, 1, 0.0f);
    if (send_clip_table(*cc.tab, (size_t)num_frames, tg.s) != 0) return -1;
    if (natives) {
        for (int b0 = 0; b0 < num_frames; b0 += per_batch)
            if (clip_native_batch(cc, b0, std::min(per_batch, num_frames - b0)) != 0) return -1;
        return 0;
    }
    void *params[] = {&cc.a, &cc.xy, &cc.c};
    return clip_call_run(cc, num_frames, per_batch, 1, params, &inv->clip_batched_launches);
}

int mmhip_render_clip(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int region_x, int region_y,
                      int region_w, int region_h, int first_row, int last_row, void *out_device, int row_stride,
                      int64_t frame_stride, int bpp, int floatmap, void *stream) {
    ClipTarget tg;
    const int go = clip_target("render_clip", inv, 0.0f, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row,
                               out_device, row_stride, frame_stride, bpp, floatmap, stream, false, &tg);
    return go == 1 ? render_clip_to(inv, tg, num_frames, frames, ts) : go;
}

// ---- supersampled clips ----
// How mmhip_render_clip_supersampled cuts a clip into batches.  Frames per batch: what both slices' clip launches take
// in one launch each (clip_plan of the region_w + 1 and the region_w geometry at that many frames), at most 65 535 (the
// combine's gridDim.y), and what MMHIP_CLIP_SS_BYTES (read once, default 2 GiB) holds of one frame's two slices.
// per_batch 0: the loop of mmhip_render_supersampled -- filters with native calls or closure images (their nested
// renders rely on the native memo across the two slices), and frames too large for any of the above.
struct ClipSsPlan { int per_batch = 0; size_t bytes_per_frame = 0, long_pitch = 0; };
static ClipSsPlan clip_ss_plan(const mmhip_filter *f, bool host_between, int region_w, int region_h, int bpp, int frames) {
    static const size_t budget = env_bytes("MMHIP_CLIP_SS_BYTES", (size_t)2 << 30);
    ClipSsPlan p;
    p.long_pitch = supersample_clip_long_pitch(region_w, bpp);
    p.bytes_per_frame = (size_t)region_h * (p.long_pitch + (size_t)region_w * bpp);
    if (host_between || region_w == INT32_MAX || p.long_pitch > (size_t)INT32_MAX || supersample_clip_items(region_w, region_h) > INT32_MAX)
        return p;
    long per = (long)std::min<size_t>({(size_t)frames, (size_t)65535, budget / p.bytes_per_frame});
    // fewer frames in a launch may mean fewer rows per work-item, more workgroups per frame and a lower cap
    while (per > 0) {
        const int cap = std::min(clip_plan(clip_launch_geometry(f->ks, region_w + 1, region_h, (int)per)).max_frames,
                                 clip_plan(clip_launch_geometry(f->ks, region_w, region_h, (int)per)).max_frames);
        if (cap >= per) break;
        per = cap;
    }
    p.per_batch = (int)per;
    return p;
}

int mmhip_filter_clip_supersample_plan(const mmhip_filter *f, int region_w, int region_h, int bpp, int frames, int64_t *out) {
    if (frames < 1) return fail("clip supersample plan: num_frames must be at least 1");
    if (bpp < 1 || bpp > 4) return fail("output_bpp must be 1..4");
    if (region_w < 1 || region_h < 1) return fail("clip supersample plan: empty region");
    const ClipSsPlan p = clip_ss_plan(f, !f->ks.natives.empty() || !f->closures.empty(), region_w, region_h, bpp, frames);
    const int64_t v[MMHIP_CLIP_SS_PLAN_FIELDS] = {p.per_batch > 0, p.per_batch, p.per_batch ? (frames + p.per_batch - 1) / p.per_batch : 0,
                                                  (int64_t)p.bytes_per_frame, (int64_t)p.long_pitch, SS_CLIP_ROWS, SS_CLIP_PIXELS};
    memcpy(out, v, sizeof v);
    return 0;
}

long mmhip_clip_supersampled_batches(mmhip_invocation *inv) { return inv->clip_supersampled_batches; }

int mmhip_render_clip_supersampled(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int region_x,
                                   int region_y, int region_w, int region_h, void *out_device, int row_stride,
                                   int64_t frame_stride, int bpp, void *stream) {
    if (check_clip_args("render_clip_supersampled", num_frames, frames, ts, bpp, region_w, region_h) != 0) return -1;
    if (check_frame_stride("render_clip_supersampled", inv, frame_stride, region_h, region_w, row_stride, bpp, 0) != 0) return -1;
    const bool host_between = !inv->f->ks.natives.empty() || !inv->f->closures.empty();
    const ClipSsPlan plan = clip_ss_plan(host_between ? inv->f : active_filter(inv, frames[0], ts[0]), host_between, region_w,
                                         region_h, bpp, num_frames);
    if (plan.per_batch < 1) {
        for (int i = 0; i < num_frames; ++i)
            if (mmhip_render_supersampled(inv, frames[i], ts[i], region_x, region_y, region_w, region_h,
                                          (char *)out_device + (int64_t)i * frame_stride, row_stride, bpp, stream) != 0)
                return -1;
        return 0;
    }
    hipStream_t s = stream ? (hipStream_t)stream : inv->stream;
    const int per_batch = plan.per_batch;
    const size_t long_frame = (size_t)region_h * plan.long_pitch, short_frame = (size_t)region_h * region_w * bpp;
    // own allocation, like ss_lines; whatever still reads a smaller one has finished before it is freed
    if (inv->clip_ss.grow((size_t)per_batch * plan.bytes_per_frame, hipDeviceSynchronize) != hipSuccess)
        return fail("out of device memory for the supersampling slices of a clip; lower MMHIP_CLIP_SS_BYTES");
    unsigned char *longs = inv->clip_ss.get<unsigned char>(), *shorts = longs + (size_t)per_batch * long_frame;
    SamplingOffsetGuard offsets(inv);
    for (int b0 = 0; b0 < num_frames; b0 += per_batch) {
        const int n = std::min(per_batch, num_frames - b0);
        // long slices: region_width + 1 columns at offsets -0.5, then the short ones at 0 (mmhip_render_supersampled)
        offsets.set(-0.5f);
        if (mmhip_render_clip(inv, n, frames + b0, ts + b0, region_x, region_y, region_w + 1, region_h, region_y, region_y + region_h,
                              longs, (int)plan.long_pitch, (int64_t)long_frame, bpp, 0, s) != 0)
            return -1;
        offsets.set(0.f);
        if (mmhip_render_clip(inv, n, frames + b0, ts + b0, region_x, region_y, region_w, region_h, region_y, region_y + region_h,
                              shorts, region_w * bpp, (int64_t)short_frame, bpp, 0, s) != 0)
            return -1;
        std::string err;
        if (launch_supersample_combine_clip(longs, shorts, (unsigned char *)out_device + (int64_t)b0 * frame_stride, region_w, region_h,
                                            bpp, row_stride, frame_stride, n, inv->ws, s, &err) != 0)
            return fail(err);
        ++inv->clip_supersampled_batches;
    }
    return 0;
}

// ---- clips through sub-sample maps: motion-blurred (mmhip_render_clip_shutter), grid-supersampled (mmhip_render_clip_sampled) ----
// MMHIP_CLIP_SHUTTER_BYTES is read once, default 8 GiB.
static size_t clip_shutter_budget() {
    static const size_t budget = env_bytes("MMHIP_CLIP_SHUTTER_BYTES", (size_t)8 << 30);
    return budget;
}

// How the maps path cuts a clip into batches and a frame's time steps into passes (include/mmhip.h has the rules of both
// entry points): `samples` time steps of `grid` maps each -- one for the shutter alone -- under the one budget.
struct ClipMapsPlan { int per_batch = 1, batches = 1, steps_per_pass = 1, passes = 1, carry = 0; size_t bytes_per_sample = 0; };
static ClipMapsPlan clip_maps_plan(int num_rows, int render_w, int samples, int grid, int frames) {
    const size_t budget = clip_shutter_budget();
    ClipMapsPlan p;
    p.bytes_per_sample = (size_t)num_rows * 16 * (size_t)render_w;
    const size_t frame_bytes = (size_t)samples * grid * p.bytes_per_sample;
    if (budget >= frame_bytes) {
        p.per_batch = (int)std::min<size_t>({budget / frame_bytes, (size_t)65535, (size_t)frames});
        p.steps_per_pass = samples;
    } else {
        // not one frame's sub-samples: a frame at a time, in passes of whole time steps beside the carry map (at least one step)
        p.steps_per_pass = (int)std::max<long long>(1, ((long long)(budget / p.bytes_per_sample) - 1) / grid);
        p.passes = (samples + p.steps_per_pass - 1) / p.steps_per_pass;
        p.carry = p.passes > 1;
    }
    p.batches = (frames + p.per_batch - 1) / p.per_batch;
    return p;
}

static int clip_shutter_check_samples(const char *who, int samples) {
    if (samples < 1 || samples > MMHIP_SHUTTER_MAX_SAMPLES)
        return fail(std::string(who) + ": samples must be 1 to " + std::to_string((int)MMHIP_SHUTTER_MAX_SAMPLES) + ", not " + std::to_string(samples));
    return 0;
}

// The checks the sampled entry points make of the grid and the sub-sample count, under the name of the one called.
static int clip_sampled_check(const char *who, int samples, int grid_x, int grid_y) {
    if (grid_x < 1 || grid_x > MMHIP_SAMPLE_GRID_MAX || grid_y < 1 || grid_y > MMHIP_SAMPLE_GRID_MAX)
        return fail(std::string(who) + ": grid_x and grid_y must be 1 to " + std::to_string((int)MMHIP_SAMPLE_GRID_MAX) + ", not " +
                    std::to_string(grid_x) + " x " + std::to_string(grid_y));
    if (clip_shutter_check_samples(who, samples) != 0) return -1;
    if (samples * grid_x * grid_y > MMHIP_SHUTTER_MAX_SAMPLES)
        return fail(std::string(who) + ": samples * grid_x * grid_y must be at most " + std::to_string((int)MMHIP_SHUTTER_MAX_SAMPLES) + ", not " +
                    std::to_string(samples * grid_x * grid_y));
    return 0;
}

// The fields both maps plans report (MMHIP_CLIP_SHUTTER_PLAN_FIELDS, MMHIP_CLIP_SAMPLED_PLAN_FIELDS: the same six).
static int put_maps_plan(const ClipMapsPlan &p, int64_t *out) {
    static_assert(MMHIP_CLIP_SHUTTER_PLAN_FIELDS == 6 && MMHIP_CLIP_SAMPLED_PLAN_FIELDS == 6, "the maps plans' fields");
    const int64_t v[6] = {p.per_batch, p.batches, p.steps_per_pass, p.passes, (int64_t)p.bytes_per_sample, p.carry};
    memcpy(out, v, sizeof v);
    return 0;
}

int mmhip_filter_clip_shutter_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int samples, int frames, int64_t *out) {
    (void)f;
    if (frames < 1) return fail("clip shutter plan: num_frames must be at least 1");
    if (clip_shutter_check_samples("clip shutter plan", samples) != 0) return -1;
    if (region_w < 1 || num_rows < 1 || render_w < region_w) return fail("clip shutter plan: empty region, or one wider than the render width");
    return put_maps_plan(clip_maps_plan(num_rows, render_w, samples, 1, frames), out);
}

int mmhip_filter_clip_sampled_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int samples, int grid_x, int grid_y,
                                   int frames, int64_t *out) {
    (void)f;
    if (frames < 1) return fail("clip sampled plan: num_frames must be at least 1");
    if (clip_sampled_check("clip sampled plan", samples, grid_x, grid_y) != 0) return -1;
    if (region_w < 1 || num_rows < 1 || render_w < region_w) return fail("clip sampled plan: empty region, or one wider than the render width");
    return put_maps_plan(clip_maps_plan(num_rows, render_w, samples, grid_x * grid_y, frames), out);
}

long mmhip_clip_shutter_batches(mmhip_invocation *inv) { return inv->clip_shutter_batches; }
long mmhip_clip_sampled_batches(mmhip_invocation *inv) { return inv->clip_sampled_batches; }

// A clip of frames that are each the mean of samples * grid_x * grid_y float maps: `samples` instants of the shutter, at
// every one a grid_x x grid_y grid of sampling offsets inside the pixel.  A 1 x 1 grid is the motion-blurred clip and
// renders at the caller's sampling offset, which it does not touch; a grid replaces that offset with its own and puts it
// back on every way out.  The two speak and count as the entry points they are.
static int render_clip_maps(mmhip_invocation *inv, const ClipTarget &tg, int num_frames, const int *frames, const float *ts, int samples,
                            float span, int grid_x, int grid_y) {
    const int grid = grid_x * grid_y;
    const bool gridded = grid > 1;
    const std::string who = gridded ? "render_clip_sampled" : "render_clip_shutter";
    long &batches = gridded ? inv->clip_sampled_batches : inv->clip_shutter_batches;
    const ClipMapsPlan plan = clip_maps_plan(tg.num_rows, inv->render_w, samples, grid, num_frames);
    const size_t bps = plan.bytes_per_sample;
    if (bps > ((size_t)1 << 32)) return fail(who + ": a sub-sample map of more than 4 GiB; render the frame in row bands");
    hipStream_t s = tg.s;
    // own allocation, like clip_ss: [frame][time step][grid point] maps, the carry map behind them; whatever still reads a
    // smaller one has finished before it is freed
    const size_t slots = (size_t)plan.per_batch * plan.steps_per_pass * grid;
    if (inv->clip_shutter.grow((slots + plan.carry) * bps, hipDeviceSynchronize) != hipSuccess)
        return fail(std::string("out of device memory for the sub-samples of a ") + (gridded ? "grid-supersampled" : "motion-blurred") +
                    " clip; lower MMHIP_CLIP_SHUTTER_BYTES");
    unsigned char *subs = inv->clip_shutter.get<unsigned char>(), *carry = plan.carry ? subs + slots * bps : nullptr;
    const float inv_k = mm_shutter_inv_k(samples * grid);
    SamplingOffsetGuard offsets(inv);
    std::vector<int> sub_frames;
    std::vector<float> sub_ts;
    for (int b0 = 0; b0 < num_frames; b0 += plan.per_batch) {
        const int n = std::min(plan.per_batch, num_frames - b0);
        for (int j0 = 0; j0 < samples; j0 += plan.steps_per_pass) {
            const int count = std::min(plan.steps_per_pass, samples - j0);
            sub_frames.resize((size_t)n * count);
            sub_ts.resize((size_t)n * count);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < count; ++j) {
                    sub_frames[(size_t)i * count + j] = frames[b0 + i];
                    sub_ts[(size_t)i * count + j] = mm_shutter_sample_t(ts[b0 + i], span, j0 + j, samples);
                }
            // grid point g = b * grid_x + a of entry e = i * count + j lands at (e * G + g) * bps: the layout [i][j][g]
            for (int b = 0; b < grid_y; ++b)
                for (int a = 0; a < grid_x; ++a) {
                    if (gridded) offsets.set(mm_sample_grid_offset(a, grid_x), mm_sample_grid_offset(b, grid_y));
                    if (render_clip_to(inv, tg.as_floatmaps(subs + (size_t)(b * grid_x + a) * bps, (int64_t)grid * (int64_t)bps), n * count,
                                       sub_frames.data(), sub_ts.data()) != 0)
                        return -1;
                }
            const bool last = j0 + count >= samples;
            std::string err;
            const ClipSamples in{subs, (int64_t)bps, (int64_t)count * grid * (int64_t)bps, count * grid, j0 > 0 ? carry : nullptr, last ? nullptr : carry};
            if (launch_shutter_combine_clip(in, tg.from_frame(b0).store(), tg.region_w, tg.num_rows, inv->render_w, inv_k, n, inv->ws, s, &err) != 0)
                return fail(err);
        }
        ++batches;
    }
    return 0;
}

int mmhip_render_clip_shutter(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples, float span,
                              int region_x, int region_y, int region_w, int region_h, int first_row, int last_row, void *out_device,
                              int row_stride, int64_t frame_stride, int bpp, int floatmap, void *stream) {
    const char *who = "render_clip_shutter";
    if (clip_shutter_check_samples(who, samples) != 0) return -1;
    if (samples == 1)       // one instant per frame: the plain clip itself
        return mmhip_render_clip(inv, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                                 row_stride, frame_stride, bpp, floatmap, stream);
    ClipTarget tg;
    const int go = clip_target(who, inv, span, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                               row_stride, frame_stride, bpp, floatmap, stream, true, &tg);
    return go == 1 ? render_clip_maps(inv, tg, num_frames, frames, ts, samples, span, 1, 1) : go;
}

int mmhip_render_clip_sampled(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples, float span,
                              int grid_x, int grid_y, int region_x, int region_y, int region_w, int region_h, int first_row,
                              int last_row, void *out_device, int row_stride, int64_t frame_stride, int bpp, int floatmap, void *stream) {
    const char *who = "render_clip_sampled";
    if (grid_x == 1 && grid_y == 1)      // one sample per pixel: the motion-blurred clip itself (and with samples = 1 the plain one)
        return mmhip_render_clip_shutter(inv, num_frames, frames, ts, samples, span, region_x, region_y, region_w, region_h, first_row,
                                         last_row, out_device, row_stride, frame_stride, bpp, floatmap, stream);
    if (clip_sampled_check(who, samples, grid_x, grid_y) != 0) return -1;
    ClipTarget tg;
    const int go = clip_target(who, inv, span, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                               row_stride, frame_stride, bpp, floatmap, stream, true, &tg);
    return go == 1 ? render_clip_maps(inv, tg, num_frames, frames, ts, samples, span, grid_x, grid_y) : go;
}

// ---- grid-supersampled clips under a reconstruction filter wider than a pixel (mmhip_render_clip_filtered) ----
static int clip_filter_check(const char *who, int kernel, float radius) {
    if (kernel < 0 || kernel >= MM_CLIP_FILTER_KERNELS)
        return fail(std::string(who) + ": kernel must be MMHIP_AA_BOX, MMHIP_AA_TENT, MMHIP_AA_GAUSSIAN or MMHIP_AA_MITCHELL (0 to 3), not " +
                    std::to_string(kernel));
    if (!std::isfinite(radius) || radius < 0.5f || radius > 4.0f)
        return fail(std::string(who) + ": radius must be 0.5 to 4 pixels, not " + std::to_string(radius));
    return 0;
}

// The rectangle the sub-sample maps of a filtered clip hold: the output's columns and rows and the D neighbours either
// side of them that lie inside the frame.
struct ClipHalo { int x0, y0, w, rows; };
static ClipHalo clip_halo(int region_x, int region_w, int first_row, int last_row, int render_w, int render_h, int reach) {
    ClipHalo h;
    h.x0 = std::max(0, region_x - reach);
    h.y0 = std::max(0, first_row - reach);
    h.w = (int)std::min<int64_t>(render_w, (int64_t)region_x + region_w + reach) - h.x0;
    h.rows = (int)std::min<int64_t>(render_h, (int64_t)last_row + reach) - h.y0;
    return h;
}

// The rectangle of a filtered call inside the frame?  (the rows are clamped to the region already)
static int clip_filtered_check_rect(const char *who, int region_x, int region_w, int first_row, int last_row, int render_w, int render_h) {
    if (region_x < 0 || (int64_t)region_x + region_w > render_w)
        return fail(std::string(who) + ": the region's columns [" + std::to_string(region_x) + ", " + std::to_string((int64_t)region_x + region_w) +
                    ") must lie inside the render width " + std::to_string(render_w));
    if (first_row < 0 || last_row > render_h)
        return fail(std::string(who) + ": the rows [" + std::to_string(first_row) + ", " + std::to_string(last_row) +
                    ") must lie inside the render height " + std::to_string(render_h));
    return 0;
}

int mmhip_clip_filter_taps(int kernel, float radius, int n, int lo, int hi, float *out) {
    const char *who = "clip_filter_taps";
    if (clip_filter_check(who, kernel, radius) != 0) return -1;
    const int reach = mm_clip_filter_reach((double)radius);
    if (n < 1 || n > MMHIP_SAMPLE_GRID_MAX) return fail(std::string(who) + ": n must be 1 to " + std::to_string((int)MMHIP_SAMPLE_GRID_MAX) + ", not " + std::to_string(n));
    if (lo < 0 || lo > reach || hi < 0 || hi > reach)
        return fail(std::string(who) + ": lo and hi must be 0 to D = " + std::to_string(reach) + ", not " + std::to_string(lo) + " and " + std::to_string(hi));
    if (!out) return fail(std::string(who) + ": out must hold (2 D + 1) * n floats");
    float offs[MM_SAMPLE_GRID_MAX];
    for (int a = 0; a < n; ++a) offs[a] = mm_sample_grid_offset(a, n);
    if (mm_clip_filter_taps(kernel, (double)radius, n, offs, lo, hi, out) != 0)
        return fail(std::string(who) + ": the weights do not sum to a positive finite number");
    return mm_clip_filter_tap_count(reach, n);
}

int mmhip_filter_clip_filtered_plan(const mmhip_filter *f, int region_x, int region_w, int first_row, int last_row, int render_w, int render_h,
                                    int samples, int grid_x, int grid_y, float radius, int frames, int64_t *out) {
    (void)f;
    const char *who = "clip filtered plan";
    if (frames < 1) return fail("clip filtered plan: num_frames must be at least 1");
    if (clip_sampled_check(who, samples, grid_x, grid_y) != 0) return -1;
    if (clip_filter_check(who, MM_CLIP_FILTER_BOX, radius) != 0) return -1;
    if (region_w < 1 || last_row <= first_row || render_w < 1 || render_h < 1) return fail("clip filtered plan: empty region");
    if (clip_filtered_check_rect(who, region_x, region_w, first_row, last_row, render_w, render_h) != 0) return -1;
    const ClipHalo h = clip_halo(region_x, region_w, first_row, last_row, render_w, render_h, mm_clip_filter_reach((double)radius));
    const ClipMapsPlan p = clip_maps_plan(h.rows, render_w, samples, grid_x * grid_y, frames);
    static_assert(MMHIP_CLIP_FILTERED_PLAN_FIELDS == 8, "the filtered plan's fields");
    const int64_t v[8] = {p.per_batch, p.batches, p.steps_per_pass, p.passes, (int64_t)p.bytes_per_sample, p.carry, h.w, h.rows};
    memcpy(out, v, sizeof v);
    return 0;
}

long mmhip_clip_filtered_batches(mmhip_invocation *inv) { return inv->clip_filtered_batches; }

// The tap blocks of one axis of `size` pixels with n grid points, for every edge class, appended to `out`.
static int clip_filter_blocks(const char *who, int kernel, float radius, int n, int size, std::vector<unsigned> *out) {
    const int reach = mm_clip_filter_reach((double)radius);
    const size_t at = out->size();
    out->resize(at + (size_t)(reach + 1) * (reach + 1) * mm_clip_filter_block_words(mm_clip_filter_tap_count(reach, n)));
    float offs[MM_SAMPLE_GRID_MAX];
    for (int a = 0; a < n; ++a) offs[a] = mm_sample_grid_offset(a, n);
    if (mm_clip_filter_axis_blocks(kernel, (double)radius, n, offs, size, out->data() + at) != 0)
        return fail(std::string(who) + ": the filter's weights do not sum to a positive finite number");
    return 0;
}

int mmhip_render_clip_filtered(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples, float span, int grid_x,
                               int grid_y, int kernel, float radius, int region_x, int region_y, int region_w, int region_h, int first_row,
                               int last_row, void *out_device, int row_stride, int64_t frame_stride, int bpp, int floatmap, void *stream) {
    const char *who = "render_clip_filtered";
    if (clip_sampled_check(who, samples, grid_x, grid_y) != 0) return -1;
    if (clip_filter_check(who, kernel, radius) != 0) return -1;
    ClipTarget tg;
    const int go = clip_target(who, inv, span, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                               row_stride, frame_stride, bpp, floatmap, stream, true, &tg);
    if (go != 1) return go;
    const int render_w = inv->render_w, render_h = inv->render_h;
    if (clip_filtered_check_rect(who, tg.region_x, tg.region_w, tg.first_row, tg.last_row, render_w, render_h) != 0) return -1;
    const int grid = grid_x * grid_y, reach = mm_clip_filter_reach((double)radius);
    const ClipHalo halo = clip_halo(tg.region_x, tg.region_w, tg.first_row, tg.last_row, render_w, render_h, reach);
    const ClipMapsPlan plan = clip_maps_plan(halo.rows, render_w, samples, grid, num_frames);
    const size_t bps = plan.bytes_per_sample;
    if (bps > ((size_t)1 << 32))
        return fail(std::string(who) + ": a sub-sample map of the haloed rectangle of more than 4 GiB; render the frame in row bands");
    hipStream_t s = tg.s;
    // the tap tables of both axes: built here, one upload per call
    std::vector<unsigned> &tables = inv->clip_filter_host;
    tables.clear();
    if (clip_filter_blocks(who, kernel, radius, grid_x, render_w, &tables) != 0) return -1;
    const size_t y_tables = tables.size();
    if (clip_filter_blocks(who, kernel, radius, grid_y, render_h, &tables) != 0) return -1;
    HIP_TRY(inv->clip_filter_taps.grow(tables.size() * sizeof(unsigned), [s] { return hipStreamSynchronize(s); }));
    HIP_TRY(hipMemcpyAsync(inv->clip_filter_taps.get(), tables.data(), tables.size() * sizeof(unsigned), hipMemcpyHostToDevice, s));
    const unsigned *wx = inv->clip_filter_taps.get<unsigned>(), *wy = wx + y_tables;
    const ClipFilterTaps taps{grid_x, grid_y, reach, wx, wy};
    const ClipRect rect{tg.region_x, tg.first_row, tg.region_w, tg.num_rows, halo.x0, halo.y0, halo.w, halo.rows, render_w, render_h};
    // the shutter's temporary: [frame][time step][grid point] maps of the haloed rectangle, the carry map of the output
    // rectangle (smaller than a map) behind them; whatever still reads a smaller one has finished before it is freed
    const size_t slots = (size_t)plan.per_batch * plan.steps_per_pass * grid;
    if (inv->clip_shutter.grow((slots + plan.carry) * bps, hipDeviceSynchronize) != hipSuccess)
        return fail("out of device memory for the sub-samples of a filtered clip; lower MMHIP_CLIP_SHUTTER_BYTES");
    unsigned char *subs = inv->clip_shutter.get<unsigned char>(), *carry = plan.carry ? subs + slots * bps : nullptr;
    const float inv_k = mm_shutter_inv_k(samples);
    // what the nested renders land in: the haloed rectangle as float maps
    ClipTarget maps = tg;
    maps.region_x = halo.x0;
    maps.region_y = halo.y0;
    maps.region_w = halo.w;
    maps.region_h = halo.rows;
    maps.first_row = halo.y0;
    maps.last_row = halo.y0 + halo.rows;
    maps.num_rows = halo.rows;
    SamplingOffsetGuard offsets(inv);
    std::vector<int> sub_frames;
    std::vector<float> sub_ts;
    for (int b0 = 0; b0 < num_frames; b0 += plan.per_batch) {
        const int n = std::min(plan.per_batch, num_frames - b0);
        for (int j0 = 0; j0 < samples; j0 += plan.steps_per_pass) {
            const int count = std::min(plan.steps_per_pass, samples - j0);
            sub_frames.resize((size_t)n * count);
            sub_ts.resize((size_t)n * count);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < count; ++j) {
                    sub_frames[(size_t)i * count + j] = frames[b0 + i];
                    sub_ts[(size_t)i * count + j] = mm_shutter_sample_t(ts[b0 + i], span, j0 + j, samples);
                }
            // the layout [i][j][g] of render_clip_maps
            for (int b = 0; b < grid_y; ++b)
                for (int a = 0; a < grid_x; ++a) {
                    offsets.set(mm_sample_grid_offset(a, grid_x), mm_sample_grid_offset(b, grid_y));
                    if (render_clip_to(inv, maps.as_floatmaps(subs + (size_t)(b * grid_x + a) * bps, (int64_t)grid * (int64_t)bps), n * count,
                                       sub_frames.data(), sub_ts.data()) != 0)
                        return -1;
                }
            const bool last = j0 + count >= samples;
            std::string err;
            const ClipSamples in{subs, (int64_t)bps, (int64_t)count * grid * (int64_t)bps, count, j0 > 0 ? carry : nullptr, last ? nullptr : carry};
            if (launch_filter_combine_clip(in, taps, tg.from_frame(b0).store(), rect, inv_k, n, inv->ws, s, &err) != 0) return fail(err);
        }
        ++inv->clip_filtered_batches;
    }
    return 0;
}

// ---- the same clips, fused: a pixel's sub-samples summed in the pixel kernel's registers ----
// mm_shutter of mm_pixels_shutter (hipgen.cpp shutter_prelude)
struct HShutter { int samples; float inv_k; };
static_assert(sizeof(HShutter) == 8, "mm_shutter layout");
// mm_sampled of the sampled variant's kernels (hipgen.cpp sampled_prelude)
struct HSampled { const float *offs; float *xtabs; float *ytabs; int samples, gx, gy, total; float inv_k; int pad; };
static_assert(sizeof(HSampled) == 48, "mm_sampled layout");

// How mmhip_render_clip_shutter_fused cuts a clip into batches (include/mmhip.h has the rules): a slot is one sub-sample's
// frame constants and row table, per_batch output frames are one pixel launch.  fused false: the call is
// mmhip_render_clip_shutter.
struct ClipShutterFusedPlan {
    bool fused = false, per_frame = false;
    int per_batch = 0, batches = 0, slots_per_batch = 0;
    long grid_x = 0;
    LaunchGeometry geo;
    size_t xy_stride = 0, rowtab_stride = 0;      // of one slot: bytes, floats
};
static ClipShutterFusedPlan clip_shutter_fused_plan(const mmhip_filter *f, int region_w, int num_rows, int samples, int frames) {
    ClipShutterFusedPlan p;
    p.geo = single_pixel_launch_geometry(f->ks, region_w, num_rows);
    const ClipPlan cp = clip_plan(p.geo);
    p.grid_x = cp.grid_x;
    p.per_frame = f->ks.prologue_uses_time;
    p.xy_stride = ((size_t)std::max(f->ks.xy_bytes, 256) + 255) / 256 * 256;
    p.rowtab_stride = (size_t)f->ks.row_values * num_rows;
    if (!f->ks.natives.empty() || !f->closures.empty()) return p;
    long per = std::min<long>({(long)frames, (long)(cp.max_grid_rows / samples), cp.max_rows_by_items});
    if (p.per_frame) {
        per = std::min<long>(per, (long)((size_t)INT32_MAX / (p.xy_stride * samples)));
        if (p.rowtab_stride) per = std::min<long>(per, (long)((size_t)INT32_MAX / (p.rowtab_stride * samples)));
    }
    if (per < 1) return p;
    p.fused = true;
    p.per_batch = (int)per;
    p.batches = (frames + p.per_batch - 1) / p.per_batch;
    p.slots_per_batch = p.per_frame ? p.per_batch * samples : 1;
    return p;
}

// How mmhip_render_clip_sampled_fused cuts a clip into batches: the fused shutter's plan with K * G sub-samples per pixel
// and K slots per frame.  fused false: the call is mmhip_render_clip_sampled.
static ClipShutterFusedPlan clip_sampled_fused_plan(const mmhip_filter *f, int region_w, int num_rows, int samples, int grid_x, int grid_y, int frames) {
    ClipShutterFusedPlan p = clip_shutter_fused_plan(f, region_w, num_rows, samples, frames);
    // the per-row slice's values follow y: such filters take the maps path; so do regions whose tables an int does not index
    if (p.fused && (f->ks.row_values > 0 || (int64_t)grid_x * region_w > INT32_MAX || (int64_t)grid_y * num_rows > INT32_MAX)) {
        p.fused = false;
        p.per_batch = p.batches = p.slots_per_batch = 0;
    }
    return p;
}

// The fields both fused plans report (MMHIP_CLIP_SHUTTER_FUSED_PLAN_FIELDS, MMHIP_CLIP_SAMPLED_FUSED_PLAN_FIELDS: the same five).
static int put_fused_plan(const ClipShutterFusedPlan &p, int64_t *out) {
    static_assert(MMHIP_CLIP_SHUTTER_FUSED_PLAN_FIELDS == 5 && MMHIP_CLIP_SAMPLED_FUSED_PLAN_FIELDS == 5, "the fused plans' fields");
    const int64_t v[5] = {p.fused, p.per_batch, p.batches, p.fused ? p.slots_per_batch : 0, p.grid_x};
    memcpy(out, v, sizeof v);
    return 0;
}

int mmhip_filter_clip_shutter_fused_plan(const mmhip_filter *f, int region_w, int num_rows, int samples, int frames, int64_t *out) {
    if (frames < 1) return fail("clip shutter fused plan: num_frames must be at least 1");
    if (clip_shutter_check_samples("clip shutter fused plan", samples) != 0) return -1;
    if (region_w < 1 || num_rows < 1) return fail("clip shutter fused plan: empty region");
    return put_fused_plan(clip_shutter_fused_plan(f, region_w, num_rows, samples, frames), out);
}

int mmhip_filter_clip_sampled_fused_plan(const mmhip_filter *f, int region_w, int num_rows, int samples, int grid_x, int grid_y, int frames,
                                         int64_t *out) {
    if (frames < 1) return fail("clip sampled fused plan: num_frames must be at least 1");
    if (clip_sampled_check("clip sampled fused plan", samples, grid_x, grid_y) != 0) return -1;
    if (region_w < 1 || num_rows < 1) return fail("clip sampled fused plan: empty region");
    return put_fused_plan(grid_x * grid_y == 1 ? clip_shutter_fused_plan(f, region_w, num_rows, samples, frames)
                                               : clip_sampled_fused_plan(f, region_w, num_rows, samples, grid_x, grid_y, frames), out);
}

long mmhip_clip_shutter_fused_batches(mmhip_invocation *inv) { return inv->clip_shutter_fused_batches; }
long mmhip_clip_sampled_fused_batches(mmhip_invocation *inv) { return inv->clip_sampled_fused_batches; }

// A fused call of the variant `which`, as its plan has it (grid_x: of the pixel launch).
static ClipCall fused_clip_call(mmhip_invocation *inv, mmhip_filter *f, int which, const ClipShutterFusedPlan &plan, long grid_x,
                                const ClipTarget &tg, const int *frames, const float *ts) {
    return ClipCall{inv, f, &f->variants[which], tg.s, plan.geo, grid_x, plan.per_frame, plan.xy_stride, plan.rowtab_stride, frames, ts};
}

// The sample grid of a call of the sampled or the refine variant: room for the per-offset x and y tables (the prologue
// fills them), and behind the `slots` {t, frame} entries of the call's table, in the same upload, the grid's offsets --
// those along x from float 0, those along y from float MM_SAMPLE_GRID_MAX.  Between clip_call_begin, which has made room
// for GRID_OFFSET_ENTRIES more entries, and send_clip_table.
static const size_t GRID_OFFSET_ENTRIES = 2 * MM_SAMPLE_GRID_MAX * sizeof(float) / sizeof(HClipFrame);
static int clip_sample_grid(ClipCall &cc, const ClipTarget &tg, size_t slots, int samples, int grid_x, int grid_y, HSampled *sm) {
    mmhip_invocation *inv = cc.inv;
    hipStream_t s = cc.s;
    const size_t xtab_floats = (size_t)grid_x * tg.region_w, ytab_floats = (size_t)grid_y * tg.num_rows;
    HIP_TRY(inv->clip_sampled.grow((xtab_floats + ytab_floats) * sizeof(float), [s] { return hipStreamSynchronize(s); }));
    float *offs = (float *)((HClipFrame *)cc.tab->host.p + slots);
    for (int k = 0; k < MM_SAMPLE_GRID_MAX; ++k) {
        offs[k] = k < grid_x ? mm_sample_grid_offset(k, grid_x) : 0.0f;
        offs[MM_SAMPLE_GRID_MAX + k] = k < grid_y ? mm_sample_grid_offset(k, grid_y) : 0.0f;
    }
    *sm = HSampled{};
    sm->offs = (const float *)(cc.tab->dev.get<HClipFrame>() + slots);
    sm->xtabs = inv->clip_sampled.get<float>();
    sm->ytabs = sm->xtabs + xtab_floats;
    sm->samples = samples;
    sm->gx = grid_x;
    sm->gy = grid_y;
    sm->total = samples * grid_x * grid_y;
    sm->inv_k = mm_shutter_inv_k(sm->total);
    return 0;
}

int mmhip_render_clip_shutter_fused(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples, float span,
                                    int region_x, int region_y, int region_w, int region_h, int first_row, int last_row,
                                    void *out_device, int row_stride, int64_t frame_stride, int bpp, int floatmap, void *stream) {
    const char *who = "render_clip_shutter_fused";
    if (clip_shutter_check_samples(who, samples) != 0) return -1;
    if (samples == 1)       // one instant per frame: the plain clip itself
        return mmhip_render_clip(inv, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                                 row_stride, frame_stride, bpp, floatmap, stream);
    ClipTarget tg;
    const int go = clip_target(who, inv, span, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                               row_stride, frame_stride, bpp, floatmap, stream, true, &tg);
    if (go != 1) return go;
    mmhip_filter *f = active_filter(inv, frames[0], ts[0]);
    const ClipShutterFusedPlan plan = clip_shutter_fused_plan(f, tg.region_w, tg.num_rows, samples, num_frames);
    if (!plan.fused)        // native calls, closure images, a frame too large for one launch: the sub-sample maps
        return render_clip_maps(inv, tg, num_frames, frames, ts, samples, span, 1, 1);
    if (mmhip_filter_jit_shutter(f, 1) < 0) return -1;
    ClipCall cc = fused_clip_call(inv, f, VARIANT_SHUTTER, plan, plan.grid_x, tg, frames, ts);
    // the {t, frame} table of every sub-sample of the call: slot i * samples + j is sub-sample j of output frame i
    const size_t slots = (size_t)num_frames * samples;
    if (clip_call_begin(cc, tg, cc.v->ks, frames[0], ts[0], (size_t)plan.slots_per_batch, slots) != 0) return -1;
    fill_clip_table((HClipFrame *)cc.tab->host.p, num_frames, frames, ts, samples, span);
    if (send_clip_table(*cc.tab, slots, tg.s) != 0) return -1;
    HShutter sh{samples, mm_shutter_inv_k(samples)};
    void *params[] = {&cc.a, &cc.xy, &cc.c, &sh};      // (the prologue and the per-row slice take the first three)
    return clip_call_run(cc, num_frames, plan.per_batch, samples, params, &inv->clip_shutter_fused_batches);
}

int mmhip_render_clip_sampled_fused(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int samples, float span,
                                    int grid_x, int grid_y, int region_x, int region_y, int region_w, int region_h, int first_row,
                                    int last_row, void *out_device, int row_stride, int64_t frame_stride, int bpp, int floatmap,
                                    void *stream) {
    const char *who = "render_clip_sampled_fused";
    if (grid_x == 1 && grid_y == 1)      // one sample per pixel: the fused motion-blurred clip itself
        return mmhip_render_clip_shutter_fused(inv, num_frames, frames, ts, samples, span, region_x, region_y, region_w, region_h, first_row,
                                               last_row, out_device, row_stride, frame_stride, bpp, floatmap, stream);
    if (clip_sampled_check(who, samples, grid_x, grid_y) != 0) return -1;
    ClipTarget tg;
    const int go = clip_target(who, inv, span, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                               row_stride, frame_stride, bpp, floatmap, stream, true, &tg);
    if (go != 1) return go;
    mmhip_filter *f = active_filter(inv, frames[0], ts[0]);
    const ClipShutterFusedPlan plan = clip_sampled_fused_plan(f, tg.region_w, tg.num_rows, samples, grid_x, grid_y, num_frames);
    if (!plan.fused)        // native calls, closure images, a per-row slice, a frame too large for one launch: the sub-sample maps
        return render_clip_maps(inv, tg, num_frames, frames, ts, samples, span, grid_x, grid_y);
    if (mmhip_filter_jit_sampled(f, 1) < 0) return -1;
    ClipCall cc = fused_clip_call(inv, f, VARIANT_SAMPLED, plan, plan.grid_x, tg, frames, ts);
    // the {t, frame} table of every time step of the call -- slot i * samples + j is step j of output frame i -- and the grid
    const size_t slots = (size_t)num_frames * samples;
    if (clip_call_begin(cc, tg, cc.v->ks, frames[0], ts[0], (size_t)plan.slots_per_batch, slots + GRID_OFFSET_ENTRIES) != 0) return -1;
    fill_clip_table((HClipFrame *)cc.tab->host.p, num_frames, frames, ts, samples, span);
    HSampled sm;
    if (clip_sample_grid(cc, tg, slots, samples, grid_x, grid_y, &sm) != 0) return -1;
    if (send_clip_table(*cc.tab, slots + GRID_OFFSET_ENTRIES, tg.s) != 0) return -1;
    // (the coordinate tables are written by the first batch's prologue and stay: they depend on the geometry alone)
    void *params[] = {&cc.a, &cc.xy, &cc.c, &sm};
    return clip_call_run(cc, num_frames, plan.per_batch, samples, params, &inv->clip_sampled_fused_batches);
}

// ---- adaptively anti-aliased clips ----
// mm_refine of mm_pixels_refine (hipgen.cpp refine_prelude)
struct HRefine { const unsigned *list; const unsigned *counts; long long list_stride; };
static_assert(sizeof(HRefine) == 24, "mm_refine layout");

// How mmhip_render_clip_adaptive cuts a clip into batches (include/mmhip.h has the rules).  list_path: the refine variant
// renders the refined pixels from lists; else the full grid-supersampled clip is rendered and the mask kernel puts the
// plain pixels back (the select path).  `fused` is the sampled variant's plan at one time step: its eligibility and caps
// are the refine variant's.
struct ClipAdaptivePlan {
    bool list_path = false;
    int per_batch = 1, batches = 1;
    size_t bytes_per_map = 0, bytes_per_frame = 0, list_entries = 0;
    long refine_grid_x = 0;
    ClipShutterFusedPlan fused;
};
static ClipAdaptivePlan clip_adaptive_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int grid_x, int grid_y, int frames,
                                           int mode) {
    const size_t budget = clip_shutter_budget();
    ClipAdaptivePlan p;
    p.bytes_per_map = (size_t)num_rows * 16 * (size_t)render_w;
    p.list_entries = (size_t)region_w * (size_t)num_rows;
    p.fused = clip_sampled_fused_plan(f, region_w, num_rows, 1, grid_x, grid_y, frames);
    // a list entry is col | rl << 16
    p.list_path = mode == MMHIP_AA_REFINE_AUTO && p.fused.fused && region_w <= 65535 && num_rows <= 65535;
    p.bytes_per_frame = p.bytes_per_map + (p.list_path ? p.list_entries * sizeof(unsigned) : 0);
    // one frame per batch even over the budget
    size_t per = std::min<size_t>({std::max<size_t>(budget / p.bytes_per_frame, 1), (size_t)65535, (size_t)frames});
    if (p.list_path) {
        // (the sampled plan's grid_x * 256 covers the rectangle, so its cap on the work-items of a launch holds for this grid too)
        p.refine_grid_x = (long)((p.list_entries + 255) / 256);
        per = std::min<size_t>(per, (size_t)p.fused.per_batch);
    }
    p.per_batch = (int)per;
    p.batches = (frames + p.per_batch - 1) / p.per_batch;
    return p;
}

int mmhip_filter_clip_adaptive_plan(const mmhip_filter *f, int region_w, int num_rows, int render_w, int grid_x, int grid_y, int frames,
                                    int64_t *out) {
    if (frames < 1) return fail("clip adaptive plan: num_frames must be at least 1");
    if (clip_sampled_check("clip adaptive plan", 1, grid_x, grid_y) != 0) return -1;
    if (region_w < 1 || num_rows < 1 || render_w < region_w) return fail("clip adaptive plan: empty region, or one wider than the render width");
    const ClipAdaptivePlan p = clip_adaptive_plan(f, region_w, num_rows, render_w, grid_x, grid_y, frames, MMHIP_AA_REFINE_AUTO);
    const int64_t v[MMHIP_CLIP_ADAPTIVE_PLAN_FIELDS] = {p.list_path, p.per_batch, p.batches, (int64_t)p.bytes_per_frame, p.refine_grid_x};
    memcpy(out, v, sizeof v);
    return 0;
}

long mmhip_clip_adaptive_batches(mmhip_invocation *inv) { return inv->clip_adaptive_batches; }

int mmhip_clip_adaptive_refined(mmhip_invocation *inv, int64_t *counts, int n) {
    if (n < 0 || (n > 0 && !counts)) return fail("clip_adaptive_refined: counts must be an array of n entries");
    const int m = std::min(n, inv->clip_adaptive_frames);
    if (m > 0) {
        std::vector<unsigned> host((size_t)m);
        HIP_TRY(hipStreamSynchronize(inv->clip_adaptive_stream));
        HIP_TRY(hipMemcpy(host.data(), inv->clip_adaptive_counts.get(), (size_t)m * sizeof(unsigned), hipMemcpyDeviceToHost));
        for (int i = 0; i < m; ++i) counts[i] = host[i];
    }
    return inv->clip_adaptive_frames;
}

// The refined pixels of the `n` frames of a batch, which `tg` begins at, from their lists: the whole set-up, table and
// prologue over the batch's slots -- every batch's, since the nested render of the base maps has rewritten the frame
// constants and the coordinate tables -- and mm_pixels_refine over a grid that covers the whole rectangle (the counts
// stay on the device).  The batch is counted by the caller, its prologue slots are not.
static int clip_adaptive_refine_batch(mmhip_invocation *inv, mmhip_filter *f, const ClipAdaptivePlan &plan, const ClipTarget &tg, int n,
                                      const int *frames, const float *ts, int grid_x, int grid_y, const unsigned *lists,
                                      const unsigned *counts) {
    ClipCall cc = fused_clip_call(inv, f, VARIANT_REFINE, plan.fused, plan.refine_grid_x, tg, frames, ts);
    // the batch's {t, frame} table and behind it the grid's offsets, as mmhip_render_clip_sampled_fused lays them out
    if (clip_call_begin(cc, tg, cc.v->ks, frames[0], ts[0], (size_t)(cc.per_frame ? plan.per_batch : 1), (size_t)n + GRID_OFFSET_ENTRIES) != 0)
        return -1;
    fill_clip_table((HClipFrame *)cc.tab->host.p, n, frames, ts, 1, 0.0f);
    HSampled sm;
    if (clip_sample_grid(cc, tg, (size_t)n, 1, grid_x, grid_y, &sm) != 0) return -1;
    if (send_clip_table(*cc.tab, (size_t)n + GRID_OFFSET_ENTRIES, tg.s) != 0) return -1;
    HRefine r{lists, counts, (long long)plan.list_entries};
    void *params[] = {&cc.a, &cc.xy, &cc.c, &sm, &r};      // (the prologue takes the first four)
    return clip_call_run(cc, n, n, 1, params, nullptr);
}

int mmhip_render_clip_adaptive(mmhip_invocation *inv, int num_frames, const int *frames, const float *ts, int grid_x, int grid_y, float threshold,
                               int mode, int region_x, int region_y, int region_w, int region_h, int first_row, int last_row, void *out_device,
                               int row_stride, int64_t frame_stride, int bpp, int floatmap, void *stream) {
    const char *who = "render_clip_adaptive";
    if (std::isnan(threshold)) return fail(std::string(who) + ": threshold must not be NaN");
    if (grid_x == 1 && grid_y == 1) {      // one sample per pixel, refined or not: the plain clip itself
        const int rc = mmhip_render_clip(inv, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                                         row_stride, frame_stride, bpp, floatmap, stream);
        if (rc == 0 && inv) inv->clip_adaptive_frames = 0;      // no mask, no counts
        return rc;
    }
    if (clip_sampled_check(who, 1, grid_x, grid_y) != 0) return -1;
    if (mode != MMHIP_AA_REFINE_AUTO && mode != MMHIP_AA_REFINE_SELECT)
        return fail(std::string(who) + ": mode must be 0 (auto) or 1 (select), not " + std::to_string(mode));
    ClipTarget tg;
    const int go = clip_target(who, inv, 0.0f, num_frames, frames, ts, region_x, region_y, region_w, region_h, first_row, last_row, out_device,
                               row_stride, frame_stride, bpp, floatmap, stream, true, &tg);
    if (go != 1) return go;
    mmhip_filter *f = active_filter(inv, frames[0], ts[0]);
    const ClipAdaptivePlan plan = clip_adaptive_plan(f, tg.region_w, tg.num_rows, inv->render_w, grid_x, grid_y, num_frames, mode);
    const size_t bps = plan.bytes_per_map;
    if (bps > ((size_t)1 << 32)) return fail(std::string(who) + ": a base map of more than 4 GiB; render the frame in row bands");
    if (plan.list_path && mmhip_filter_jit_refine(f, 1) < 0) return -1;
    hipStream_t s = tg.s;
    // own allocations (the nested grid-supersampled clip of the select path fills the shutter's temporary); whatever still
    // reads a smaller one has finished before it is freed
    if (inv->clip_adaptive.grow((size_t)plan.per_batch * plan.bytes_per_frame, hipDeviceSynchronize) != hipSuccess ||
        inv->clip_adaptive_counts.grow((size_t)num_frames * sizeof(unsigned), hipDeviceSynchronize) != hipSuccess)
        return fail("out of device memory for the base maps of an adaptively anti-aliased clip; lower MMHIP_CLIP_SHUTTER_BYTES");
    unsigned char *base = inv->clip_adaptive.get<unsigned char>();
    unsigned *lists = plan.list_path ? (unsigned *)(base + (size_t)plan.per_batch * bps) : nullptr;
    unsigned *counts = inv->clip_adaptive_counts.get<unsigned>();
    inv->clip_adaptive_frames = num_frames;
    inv->clip_adaptive_stream = s;
    SamplingOffsetGuard offsets(inv);
    offsets.set(0.f);      // the base maps are rendered at offset 0, whatever the caller's
    for (int b0 = 0; b0 < num_frames; b0 += plan.per_batch) {
        const int n = std::min(plan.per_batch, num_frames - b0);
        const ClipTarget batch = tg.from_frame(b0);
        if (render_clip_to(inv, tg.as_floatmaps(base, (int64_t)bps), n, frames + b0, ts + b0) != 0) return -1;
        // select path: every pixel refined, then the mask kernel puts back those that are not
        if (!plan.list_path && render_clip_maps(inv, batch, n, frames + b0, ts + b0, 1, 0.0f, grid_x, grid_y) != 0) return -1;
        HIP_TRY(hipMemsetAsync(counts + b0, 0, (size_t)n * sizeof(unsigned), s));
        std::string err;
        if (launch_aa_contrast_clip(base, (int64_t)bps, batch.store(), ClipRefined{counts + b0, lists, (int64_t)plan.list_entries}, tg.region_w,
                                    tg.num_rows, inv->render_w, threshold, n, inv->ws, s, &err) != 0)
            return fail(err);
        if (plan.list_path && clip_adaptive_refine_batch(inv, f, plan, batch, n, frames + b0, ts + b0, grid_x, grid_y, lists, counts + b0) != 0)
            return -1;
        ++inv->clip_adaptive_batches;
    }
    return 0;
}

// ---- clips as planar Y'CbCr 4:2:0 (mmhip_clip_to_yuv420): RGBA8 frames in HBM to Y4M payloads in HBM ----
static_assert(MMHIP_YUV_BT601 == MM_YUV_BT601 && MMHIP_YUV_BT709 == MM_YUV_BT709 && MMHIP_YUV_LIMITED == MM_YUV_LIMITED &&
                  MMHIP_YUV_FULL == MM_YUV_FULL,
              "the modes of mm_yuv.h");
int64_t mmhip_yuv420_frame_bytes(int width, int height) {
    if (width < 1 || height < 1) return fail("yuv420_frame_bytes: width and height must be at least 1");
    return mm_yuv_frame_bytes(width, height);
}

// One stream header line under the name of its entry point: the colour space tag is the only thing that varies.
static int y4m_header_line(const std::string &who, const char *tag, char *buf, int cap, int width, int height, int fps_num, int fps_den, int range) {
    if (width < 1 || height < 1) return fail(who + "width and height must be at least 1");
    if (fps_num < 1 || fps_den < 1) return fail(who + "fps_num and fps_den must be at least 1");
    if (range != MMHIP_YUV_LIMITED && range != MMHIP_YUV_FULL)
        return fail(who + "range must be MMHIP_YUV_LIMITED or MMHIP_YUV_FULL (0 or 1), not " + std::to_string(range));
    char line[160];
    const int n = snprintf(line, sizeof line, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=%s\n", width, height, fps_num, fps_den, tag,
                           range == MMHIP_YUV_FULL ? "FULL" : "LIMITED");
    if (!buf || cap < n + 1) return fail(who + "the buffer holds " + std::to_string(buf ? cap : 0) + " bytes, the header needs " + std::to_string(n + 1));
    memcpy(buf, line, (size_t)n + 1);
    return n;
}

int mmhip_y4m_header(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range) {
    return y4m_header_line("y4m_header: ", "C420jpeg", buf, cap, width, height, fps_num, fps_den, range);
}

static_assert(MMHIP_YUV_SITING_CENTER == MM_YUV_SITING_CENTER && MMHIP_YUV_SITING_LEFT == MM_YUV_SITING_LEFT, "the sitings of mm_yuv.h");
int mmhip_y4m_header_sited(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range, int bits, int siting) {
    const std::string who = "y4m_header_sited: ";
    if (bits != 8 && bits != 10) return fail(who + "bits must be 8 or 10, not " + std::to_string(bits));
    if (!mm_yuv_siting_known(siting))
        return fail(who + "siting must be MMHIP_YUV_SITING_CENTER or MMHIP_YUV_SITING_LEFT (0 or 1), not " + std::to_string(siting));
    // (Y4M has no colour space tag for left-sited 10-bit 4:2:0: C420p10 says nothing of the siting)
    const char *tag = bits == 10 ? "C420p10" : siting == MMHIP_YUV_SITING_LEFT ? "C420mpeg2" : "C420jpeg";
    return y4m_header_line(who, tag, buf, cap, width, height, fps_num, fps_den, range);
}

// One call of a converter under the name of its entry point: its refusals (they need no GPU), the invocation, the caller's
// stream or the invocation's, the launch, and the path it took counted where the converter has a counter.
template <class Job>
static int clip_yuv_convert(mmhip_invocation *inv, const Job &job, void *stream, int (*check)(const Job &, std::string *),
                            int (*launch)(const Job &, NativeWorkspace &, hipStream_t, int *, std::string *), long (mmhip_invocation::*launches)[2]) {
    std::string err;
    if (check(job, &err) != 0) return fail(err);
    if (!inv) return fail(std::string(job.name) + ": no invocation");
    hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)inv->stream;
    int path = 0;
    if (launch(job, inv->ws, s, &path, &err) != 0) return fail(err);
    if (launches) ++(inv->*launches)[path];
    return 0;
}

static int clip_to_yuv420(const char *name, mmhip_invocation *inv, const void *src_rgba, int64_t src_row_stride, int64_t src_frame_stride, int width,
                          int height, int first_row, int last_row, int num_frames, int matrix, int range, int siting, void *dst,
                          int64_t dst_frame_stride, void *stream) {
    const YuvOutJob job = {name, src_rgba, src_row_stride, src_frame_stride, width, height, first_row, last_row, num_frames, matrix, range, siting, dst,
                           dst_frame_stride};
    return clip_yuv_convert(inv, job, stream, check_rgba8_to_yuv420_clip, launch_rgba8_to_yuv420_clip, nullptr);
}

int mmhip_clip_to_yuv420(mmhip_invocation *inv, const void *src_rgba, int64_t src_row_stride, int64_t src_frame_stride, int width, int height,
                         int first_row, int last_row, int num_frames, int matrix, int range, void *dst, int64_t dst_frame_stride, void *stream) {
    return clip_to_yuv420("clip_to_yuv420", inv, src_rgba, src_row_stride, src_frame_stride, width, height, first_row, last_row, num_frames, matrix,
                          range, MMHIP_YUV_SITING_CENTER, dst, dst_frame_stride, stream);
}

int mmhip_clip_to_yuv420_sited(mmhip_invocation *inv, const void *src_rgba, int64_t src_row_stride, int64_t src_frame_stride, int width, int height,
                               int first_row, int last_row, int num_frames, int matrix, int range, int siting, void *dst,
                               int64_t dst_frame_stride, void *stream) {
    return clip_to_yuv420("clip_to_yuv420_sited", inv, src_rgba, src_row_stride, src_frame_stride, width, height, first_row, last_row, num_frames,
                          matrix, range, siting, dst, dst_frame_stride, stream);
}

// ---- clips as 10-bit planar Y'CbCr 4:2:0 (mmhip_clip_float_to_yuv420p10): float frames in HBM to Y4M payloads in HBM ----
int64_t mmhip_yuv420p10_frame_bytes(int width, int height) {
    if (width < 1 || height < 1) return fail("yuv420p10_frame_bytes: width and height must be at least 1");
    return mm_yuv10_frame_bytes(width, height);
}

int mmhip_y4m_header_p10(char *buf, int cap, int width, int height, int fps_num, int fps_den, int range) {
    return y4m_header_line("y4m_header_p10: ", "C420p10", buf, cap, width, height, fps_num, fps_den, range);
}

static int clip_float_to_yuv420p10(const char *name, mmhip_invocation *inv, const void *src, int64_t src_row_stride, int64_t src_frame_stride,
                                   int width, int height, int first_row, int last_row, int num_frames, int matrix, int range, int siting,
                                   void *dst, int64_t dst_frame_stride, void *stream) {
    const YuvOutJob job = {name, src, src_row_stride, src_frame_stride, width, height, first_row, last_row, num_frames, matrix, range, siting, dst,
                           dst_frame_stride};
    return clip_yuv_convert(inv, job, stream, check_float_to_yuv420p10_clip, launch_float_to_yuv420p10_clip, &mmhip_invocation::clip_yuv10_launches);
}

int mmhip_clip_float_to_yuv420p10(mmhip_invocation *inv, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width, int height,
                                  int first_row, int last_row, int num_frames, int matrix, int range, void *dst, int64_t dst_frame_stride,
                                  void *stream) {
    return clip_float_to_yuv420p10("clip_float_to_yuv420p10", inv, src, src_row_stride, src_frame_stride, width, height, first_row, last_row,
                                   num_frames, matrix, range, MMHIP_YUV_SITING_CENTER, dst, dst_frame_stride, stream);
}

int mmhip_clip_float_to_yuv420p10_sited(mmhip_invocation *inv, const void *src, int64_t src_row_stride, int64_t src_frame_stride, int width,
                                        int height, int first_row, int last_row, int num_frames, int matrix, int range, int siting, void *dst,
                                        int64_t dst_frame_stride, void *stream) {
    return clip_float_to_yuv420p10("clip_float_to_yuv420p10_sited", inv, src, src_row_stride, src_frame_stride, width, height, first_row, last_row,
                                   num_frames, matrix, range, siting, dst, dst_frame_stride, stream);
}

long mmhip_clip_float_to_yuv420p10_launches(mmhip_invocation *inv, int path) {
    if (path != MMHIP_YUV10_PATH_ALIGNED && path != MMHIP_YUV10_PATH_BYTES)
        return fail("clip_float_to_yuv420p10_launches: path must be MMHIP_YUV10_PATH_ALIGNED or MMHIP_YUV10_PATH_BYTES (0 or 1), not " +
                    std::to_string(path));
    return inv->clip_yuv10_launches[path];
}

// ---- planar Y'CbCr 4:2:0 as input (mmhip_clip_from_yuv420): Y4M payloads in HBM to drawable words in HBM ----
static_assert(MMHIP_YUV_CHROMA_BILINEAR == MM_YUV_CHROMA_BILINEAR && MMHIP_YUV_CHROMA_REPLICATE == MM_YUV_CHROMA_REPLICATE,
              "the chroma modes of mm_yuv.h");
static int clip_from_yuv420(const char *name, mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height,
                            int num_frames, int matrix, int range, int chroma, int siting, void *dst_rgba32, int64_t dst_frame_stride, void *stream) {
    const YuvInJob job = {name, src_yuv, src_frame_stride, width, height, num_frames, matrix, range, chroma, siting, dst_rgba32, dst_frame_stride};
    return clip_yuv_convert(inv, job, stream, check_yuv420_to_rgba_clip, launch_yuv420_to_rgba_clip, &mmhip_invocation::clip_yuv_input_launches);
}

int mmhip_clip_from_yuv420(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames, int matrix,
                           int range, int chroma, void *dst_rgba32, int64_t dst_frame_stride, void *stream) {
    return clip_from_yuv420("clip_from_yuv420", inv, src_yuv, src_frame_stride, width, height, num_frames, matrix, range, chroma,
                            MMHIP_YUV_SITING_CENTER, dst_rgba32, dst_frame_stride, stream);
}

int mmhip_clip_from_yuv420_sited(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames,
                                 int matrix, int range, int chroma, int siting, void *dst_rgba32, int64_t dst_frame_stride, void *stream) {
    return clip_from_yuv420("clip_from_yuv420_sited", inv, src_yuv, src_frame_stride, width, height, num_frames, matrix, range, chroma, siting,
                            dst_rgba32, dst_frame_stride, stream);
}

long mmhip_clip_from_yuv420_launches(mmhip_invocation *inv, int path) {
    if (path != MMHIP_YUV_IN_PATH_ALIGNED && path != MMHIP_YUV_IN_PATH_BYTES)
        return fail("clip_from_yuv420_launches: path must be MMHIP_YUV_IN_PATH_ALIGNED or MMHIP_YUV_IN_PATH_BYTES (0 or 1), not " + std::to_string(path));
    return inv->clip_yuv_input_launches[path];
}

int mmhip_clip_yuv_input_groups(mmhip_invocation *inv) { return inv->clip_yuv_input_groups; }

// The header of either depth: `bits` null refuses C420p10 with the 8-bit reader's words.
static int y4m_parse(const std::string &who, const char *buf, int len, int *width, int *height, int *fps_num, int *fps_den, int *range, int *bits,
                     int *header_len, int *siting = nullptr) {
    if (!buf || len < 0) return fail(who + "no buffer");
    const char *nl = (const char *)memchr(buf, '\n', (size_t)len);
    if (len < 9 || memcmp(buf, "YUV4MPEG2", 9) != 0 || (len > 9 && buf[9] != ' ' && buf[9] != '\n'))
        return fail(who + "the stream does not begin with the magic word YUV4MPEG2");
    if (!nl) return fail(who + "no newline within the first " + std::to_string(len) + " bytes: not a stream header");
    int w = 0, h = 0, num = 25, den = 1, rng = -1, depth = 8, sited = MMHIP_YUV_SITING_CENTER;
    // a positive int that fills the whole text, or 0
    auto number = [](const std::string &text) {
        if (text.empty() || text.size() > 9) return 0;
        for (char c : text)
            if (c < '0' || c > '9') return 0;
        return atoi(text.c_str());
    };
    const std::string line(buf + 9, nl);
    for (size_t at = 0; at < line.size();) {
        if (line[at] == ' ') { ++at; continue; }
        const size_t end = std::min(line.find(' ', at), line.size());
        const std::string tag = line.substr(at, end - at), value = tag.substr(1);
        at = end;
        switch (tag[0]) {
            case 'W': w = number(value); break;
            case 'H': h = number(value); break;
            case 'F': {
                const size_t colon = value.find(':');
                num = colon == std::string::npos ? 0 : number(value.substr(0, colon));
                den = colon == std::string::npos ? 0 : number(value.substr(colon + 1));
                if (num < 1 || den < 1) return fail(who + "the frame rate `" + tag + "' is not F<num>:<den> of positive integers");
                break;
            }
            case 'A': break;
            case 'I':
                if (value != "p" && value != "?") return fail(who + "an interlaced stream (`" + tag + "'): only progressive frames are read");
                break;
            case 'C':
                sited = value == "420mpeg2" ? MMHIP_YUV_SITING_LEFT : MMHIP_YUV_SITING_CENTER;      // (C420paldv is not modelled: centre, as it is read)
                if (bits && value == "420p10") { depth = 10; break; }
                if (value != "420jpeg" && value != "420mpeg2" && value != "420paldv" && value != "420")
                    return fail(who + "the colour space `" + tag + "' is not " +
                                (bits ? "4:2:0 of 8 or 10 bits (C420jpeg, C420mpeg2, C420paldv, C420 or C420p10)"
                                      : "8-bit 4:2:0 (C420jpeg, C420mpeg2, C420paldv or C420)"));
                depth = 8;
                break;
            case 'X':
                if (value == "COLORRANGE=FULL") rng = MMHIP_YUV_FULL;
                else if (value == "COLORRANGE=LIMITED") rng = MMHIP_YUV_LIMITED;
                break;
            default: return fail(who + "the header tag `" + tag + "' is not known");
        }
    }
    if (w < 1 || h < 1) return fail(who + "W and H must be given and positive");
    if (width) *width = w;
    if (height) *height = h;
    if (fps_num) *fps_num = num;
    if (fps_den) *fps_den = den;
    if (range) *range = rng;
    if (bits) *bits = depth;
    if (siting) *siting = sited;
    if (header_len) *header_len = (int)(nl - buf) + 1;
    return 0;
}

int mmhip_y4m_parse_header(const char *buf, int len, int *width, int *height, int *fps_num, int *fps_den, int *range, int *header_len) {
    return y4m_parse("y4m_parse_header: ", buf, len, width, height, fps_num, fps_den, range, nullptr, header_len);
}

int mmhip_y4m_parse_stream_header(const char *buf, int len, int *width, int *height, int *fps_num, int *fps_den, int *range, int *bits,
                                  int *header_len) {
    int depth = 8;
    return y4m_parse("y4m_parse_stream_header: ", buf, len, width, height, fps_num, fps_den, range, bits ? bits : &depth, header_len);
}

int mmhip_y4m_stream_siting(const char *buf, int len, int *siting) {
    int depth = 8;
    return y4m_parse("y4m_stream_siting: ", buf, len, nullptr, nullptr, nullptr, nullptr, nullptr, &depth, nullptr, siting);
}

// ---- 10-bit planar Y'CbCr 4:2:0 as input (mmhip_clip_from_yuv420p10): Y4M payloads in HBM to float4 texels in HBM ----
static int clip_from_yuv420p10(const char *name, mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height,
                               int num_frames, int matrix, int range, int chroma, int siting, void *dst_float4, int64_t dst_frame_stride,
                               void *stream) {
    const YuvInJob job = {name, src_yuv, src_frame_stride, width, height, num_frames, matrix, range, chroma, siting, dst_float4, dst_frame_stride};
    return clip_yuv_convert(inv, job, stream, check_yuv420p10_to_float_clip, launch_yuv420p10_to_float_clip,
                            &mmhip_invocation::clip_yuv10_input_launches);
}

int mmhip_clip_from_yuv420p10(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames, int matrix,
                              int range, int chroma, void *dst_float4, int64_t dst_frame_stride, void *stream) {
    return clip_from_yuv420p10("clip_from_yuv420p10", inv, src_yuv, src_frame_stride, width, height, num_frames, matrix, range, chroma,
                               MMHIP_YUV_SITING_CENTER, dst_float4, dst_frame_stride, stream);
}

int mmhip_clip_from_yuv420p10_sited(mmhip_invocation *inv, const void *src_yuv, int64_t src_frame_stride, int width, int height, int num_frames,
                                    int matrix, int range, int chroma, int siting, void *dst_float4, int64_t dst_frame_stride, void *stream) {
    return clip_from_yuv420p10("clip_from_yuv420p10_sited", inv, src_yuv, src_frame_stride, width, height, num_frames, matrix, range, chroma, siting,
                               dst_float4, dst_frame_stride, stream);
}

long mmhip_clip_from_yuv420p10_launches(mmhip_invocation *inv, int path) {
    if (path != MMHIP_YUV10_IN_PATH_ALIGNED && path != MMHIP_YUV10_IN_PATH_SAMPLES)
        return fail("clip_from_yuv420p10_launches: path must be MMHIP_YUV10_IN_PATH_ALIGNED or MMHIP_YUV10_IN_PATH_SAMPLES (0 or 1), not " +
                    std::to_string(path));
    return inv->clip_yuv10_input_launches[path];
}

int mmhip_clip_yuv10_input_groups(mmhip_invocation *inv) { return inv->clip_yuv10_input_groups; }
