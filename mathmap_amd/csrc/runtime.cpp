// C ABI + GPU runtime: hiprtc JIT, HBM-resident images and user values, launches.
//
// One mmhip_invocation corresponds to the reference's mathmap_invocation_t
// (mathmap.h:162-202): canvas/render size, user values, input drawables, edge
// behaviour.  Rendering a row band = one prologue launch (frame constants, the
// reference's init_frame, new_template.c.in:314-337) + native-filter kernels if
// the filter calls any + one pixel-kernel launch (calc_lines, :208-312).
// Clips of frames are rendered by runtime_clip.cpp.  (The exported functions have C linkage from include/mmhip.h.)
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/mmhip.h"
#include "clip_kernels.h"
#include "front.h"
#include "hipgen.h"
#include "mm_host_abi.h"
#include "native_filters.h"
#include "passes.h"
#include "runtime_internal.h"

using namespace mm;

thread_local std::string g_mmhip_err;
#define g_err g_mmhip_err

namespace {

std::string cache_dir() {
    const char *env = getenv("MMHIP_CACHE_DIR");
    std::string d = env ? env : "/tmp/mmhip-cache-" + std::to_string((int)getuid());
    mkdir(d.c_str(), 0700);
    return d;
}

}  // namespace

bool mmhip_check_options(const mmhip_options *opts) {
    if (opts && opts->gauss_mode != MMHIP_GAUSS_EXACT && opts->gauss_mode != MMHIP_GAUSS_TOLERANCE) {
        g_err = "options: gauss_mode " + std::to_string(opts->gauss_mode) + " is neither MMHIP_GAUSS_EXACT (0) nor MMHIP_GAUSS_TOLERANCE (1)";
        return false;
    }
    if (opts && opts->deep_inputs != 0 && opts->deep_inputs != 1) {
        g_err = "options: deep_inputs " + std::to_string(opts->deep_inputs) + " is neither 0 nor 1";
        return false;
    }
    if (opts && opts->deep_inputs == 1 && opts->pixel_inc > 1) {
        g_err = "options: deep_inputs with pixel_inc " + std::to_string(opts->pixel_inc) + ": the preview's stride has no meaning for float32 drawables";
        return false;
    }
    return true;
}

const char *mmhip_last_error(void) { return g_err.c_str(); }
const char *mmhip_version(void) { return "mathmap_amd 0.1 (gfx950)"; }

void mmhip_default_options(mmhip_options *o) {
    memset(o, 0, sizeof *o);
    o->intersample = 1;
    o->tile_w = 0;
}

// kernels of the closure images this filter hands to native filters (FilterCode::closure_renders)
static void generate_closure_kernels(mmhip_filter *f, const KernelOptions &ko) {
    f->closures.clear();
    for (auto &sub : f->code->closure_renders) {
        mmhip_closure_kernel ck;
        ck.ks = generate_hip(*sub, ko, f->code.get());     // may call native filters itself: render_closure runs them first
        f->closures.push_back(std::move(ck));
    }
}

static mmhip_filter *compile_source(const char *source, const mmhip_options *opts, const std::map<int, Primary> *consts, bool peel = true) {
    if (!mmhip_check_options(opts)) return nullptr;
    std::unique_ptr<mmhip_filter> f(new mmhip_filter());
    try {
        parse_module(f->module, source);
        f->source = source;
        if (opts) f->opts = *opts;
        f->code = lower_filter(f->module, f->module.main, consts);
        f->ir_json_raw = dump_ir(*f->code);
        if (consts) specialize_constants(*f->code);
        // a first loop trip that folds is peeled for kernels in exit-driven pair mode only; whether this one is shows when
        // it has been generated, so the peeled code is a trial: kept below, or the filter is compiled again without it
        const bool peeled = consts && peel && pair_peel_enabled() && peel_first_trips(*f->code);
        optimize(*f->code);
        analyze_frame_constants(*f->code);
        for (auto &sub : f->code->closure_renders) {
            if (consts) specialize_constants(*sub);
            optimize(*sub);
            eliminate_dead_cycles(*sub);
            analyze_frame_constants(*sub);
        }
        for (auto &fn : f->code->functions) optimize(*fn);     // function bodies: no frame-constant slice, no user-value literals
        KernelOptions ko;
        if (opts) {
            ko.intersample = opts->intersample;
            ko.supersampling = opts->supersampling;
            ko.edge_x = opts->edge_behaviour_x;
            ko.edge_y = opts->edge_behaviour_y;
            ko.pixel_inc = opts->pixel_inc > 1 ? opts->pixel_inc : 1;
            ko.deep_inputs = opts->deep_inputs;
            if (opts->tile_w) ko.tile_w = opts->tile_w;
            f->opts = *opts;
            f->specialize = opts->specialize_uservals != 0;
        }
        f->source = source;
        f->kopt = ko;
        f->ir_json = dump_ir(*f->code);
        f->ks = generate_hip(*f->code, ko);
        if (peeled && !f->ks.pair_exit) return compile_source(source, opts, consts, false);
        generate_closure_kernels(f.get(), ko);
    } catch (const CompileError &e) {
        g_err = e.what();
        if (e.pos >= 0) g_err += " (at offset " + std::to_string(e.pos) + ")";
        return nullptr;
    } catch (const std::exception &e) {
        g_err = e.what();
        return nullptr;
    }
    return f.release();
}

mmhip_filter *mmhip_compile(const char *source, const mmhip_options *opts) { return compile_source(source, opts, nullptr); }

// Compiles with the given scalar user values (index, value) baked in as literals -- the same
// variant active_filter() builds lazily; exposed so the specialised kernel can be inspected
// and tested without a GPU.  Values of int/bool user values are truncated to int.
static bool scalar_constants(const std::vector<UservalInfo> &uvs, int n, const int *indices, const double *values, std::map<int, Primary> *consts) {
    for (int i = 0; i < n; ++i) {
        if (indices[i] < 0 || indices[i] >= (int)uvs.size()) { g_err = "user value index out of range"; return false; }
        const UservalInfo &u = uvs[indices[i]];
        if (u.kind == UvKind::Float) (*consts)[u.index] = Primary::F((float)values[i]);
        else if (u.kind == UvKind::Int || u.kind == UvKind::Bool) (*consts)[u.index] = Primary::I((int)values[i]);
    }
    return true;
}

mmhip_filter *mmhip_compile_specialized(const char *source, const mmhip_options *opts, int n, const int *indices,
                                        const double *values) {
    Module probe;
    try {
        parse_module(probe, source);
    } catch (const std::exception &e) {
        g_err = e.what();
        return nullptr;
    }
    std::map<int, Primary> consts;
    if (!scalar_constants(probe.main->uservals, n, indices, values, &consts)) return nullptr;
    return compile_source(source, opts, &consts);
}

mmhip_filter *mmhip_filter_new_empty() { return new mmhip_filter(); }

// `f->module.main` and `f->code` have been filled in by the caller (the ABI importer).
bool mmhip_filter_finalize(mmhip_filter *f, const KernelOptions &ko, std::string *err) {
    try {
        f->code->filter = f->module.main;
        if (f->ir_json_raw.empty()) f->ir_json_raw = dump_ir(*f->code);
        optimize(*f->code);
        analyze_frame_constants(*f->code);
        for (auto &sub : f->code->closure_renders) {
            sub->filter = f->module.main;
            optimize(*sub);
            eliminate_dead_cycles(*sub);
            analyze_frame_constants(*sub);
        }
        for (auto &fn : f->code->functions) optimize(*fn);
        f->kopt = ko;
        f->ir_json = dump_ir(*f->code);
        f->ks = generate_hip(*f->code, ko);
        generate_closure_kernels(f, ko);
    } catch (const std::exception &e) {
        *err = e.what();
        return false;
    }
    return true;
}

void mmhip_filter_free(mmhip_filter *f) {
    if (!f) return;
    for (auto &p : f->spec_cache) mmhip_filter_free(p.second);
    for (mmhip_closure_kernel &ck : f->closures) if (ck.mod) (void)hipModuleUnload(ck.mod);
    if (f->mod) (void)hipModuleUnload(f->mod);
    for (ModuleVariant &v : f->variants) if (v.mod) (void)hipModuleUnload(v.mod);
    delete f;
}

const char *mmhip_filter_name(const mmhip_filter *f) { return f->module.main->name.c_str(); }
int mmhip_filter_num_uservals(const mmhip_filter *f) { return (int)f->module.main->uservals.size(); }

int mmhip_filter_userval_info(const mmhip_filter *f, int index, mmhip_userval_info *out) {
    const auto &uvs = f->module.main->uservals;
    if (index < 0 || index >= (int)uvs.size()) return fail("user value index out of range");
    const UservalInfo &u = uvs[index];
    memset(out, 0, sizeof *out);
    out->kind = (int)u.kind;
    out->index = u.index;
    snprintf(out->name, sizeof out->name, "%s", u.name.c_str());
    out->int_min = u.imin; out->int_max = u.imax; out->int_default = u.idef;
    out->float_min = u.fmin; out->float_max = u.fmax; out->float_default = u.fdef;
    out->bool_default = u.bdef;
    out->image_flags = u.image_flags;
    return 0;
}

const char *mmhip_filter_ir_json(mmhip_filter *f) { return f->ir_json.c_str(); }
const char *mmhip_filter_ir_json_raw(mmhip_filter *f) { return f->ir_json_raw.c_str(); }
const char *mmhip_filter_kernel_source(mmhip_filter *f) { return f->ks.source.c_str(); }
int mmhip_filter_gauss_mode(const mmhip_filter *f) { return f->opts.gauss_mode; }
int mmhip_filter_deep_inputs(const mmhip_filter *f) { return f->kopt.deep_inputs; }      // (what the kernels were generated with)
int mmhip_filter_num_native_calls(const mmhip_filter *f) { return f->ks.native_sites; }

int mmhip_filter_builtin_ids(const mmhip_filter *f, char *buf, int cap) {
    std::string s;
    for (const std::string &id : f->module.resolved_ids) { s += id; s += '\n'; }
    if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", s.c_str());
    return (int)s.size() + 1;
}
double mmhip_filter_jit_seconds(const mmhip_filter *f) { return f->jit_seconds; }

// hiprtc-compiles one kernel source (or fetches it from the on-disk cache); 0 on success
static int jit_source(const KernelSource &ks, std::vector<char> &code_object) {
    if (!code_object.empty()) return 0;
    // extra hiprtc options for experiments (space separated); part of the cache key
    std::vector<std::string> extra;
    std::string extra_key;
    if (const char *e = getenv("MMHIP_HIPRTC_FLAGS")) {
        std::istringstream is(e);
        for (std::string w; is >> w;) { extra.push_back(w); extra_key += "_" + std::to_string(std::hash<std::string>()(w) & 0xffff); }
    }
    if (ks.wrapping_ints) { extra.push_back("-fwrapv"); extra_key += "_wrapv"; }     // (hipgen.h: KernelSource::wrapping_ints)
    std::string path = cache_dir() + "/" + ks.key + "_o2" + extra_key + ".hsaco";   // _o2: option-set version
    std::ifstream in(path, std::ios::binary);
    const char *ov = getenv("MMHIP_SOURCE_OVERRIDE");
    const bool may_override = ov && !strncmp(ov, ks.key.c_str(), ks.key.size()) && ov[ks.key.size()] == ':';
    if (in && !getenv("MMHIP_NO_CACHE") && !may_override) code_object.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    if (!code_object.empty()) return 0;
    // kernel experiments: MMHIP_SOURCE_OVERRIDE=<key>:<file> compiles the file's text in place of the generated kernel
    // with that key (hand-edited variants of one kernel under the unchanged launch code; never cached)
    std::string source = ks.source;
    bool overridden = false;
    if (const char *e = getenv("MMHIP_SOURCE_OVERRIDE")) {
        const std::string spec = e;
        const size_t c = spec.find(':');
        if (c != std::string::npos && spec.substr(0, c) == ks.key) {
            std::ifstream f(spec.substr(c + 1));
            if (!f) return fail("MMHIP_SOURCE_OVERRIDE: cannot read " + spec.substr(c + 1));
            source.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
            overridden = true;
        }
    }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, source.c_str(), "mathmap_filter.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return fail("hiprtcCreateProgram failed");
    // -fno-slp-vectorize: the SLP vectoriser packs scalar f32 chains into v_pk_* at the price of
    // register shuffles (Mandelbrot's loop: 11 VALU with it, 10 without; measured +9 %); the
    // fetch path gets its packed math from explicit float2 code instead
    std::vector<const char *> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fno-slp-vectorize"};
    for (const std::string &w : extra) opts.push_back(w.c_str());
    hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    if (r != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, 0);
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        return fail("hiprtc compile failed:\n" + log);
    }
    size_t n = 0;
    hiprtcGetCodeSize(prog, &n);
    code_object.resize(n);
    hiprtcGetCode(prog, code_object.data());
    hiprtcDestroyProgram(&prog);
    if (overridden) return 0;
    std::string tmp = path + ".tmp" + std::to_string((int)getpid());
    std::ofstream o(tmp, std::ios::binary);
    if (o) {
        o.write(code_object.data(), (std::streamsize)code_object.size());
        o.close();
        rename(tmp.c_str(), path.c_str());
    }
    return 0;
}

// (f_rows: where the kernels have a per-row slice and the caller launches it)
static int load_kernels(const KernelSource &ks, const std::vector<char> &code_object, hipModule_t *mod, hipFunction_t *f_pix,
                        hipFunction_t *f_pro, hipFunction_t *f_rows = nullptr) {
    hipError_t e = hipModuleLoadData(mod, code_object.data());
    if (e != hipSuccess) return fail(std::string("hipModuleLoadData: ") + hipGetErrorString(e));
    e = hipModuleGetFunction(f_pix, *mod, ks.pixel_name.c_str());
    if (e != hipSuccess) return fail(std::string("hipModuleGetFunction(pixels): ") + hipGetErrorString(e));
    e = hipModuleGetFunction(f_pro, *mod, ks.prologue_name.c_str());
    if (e != hipSuccess) return fail(std::string("hipModuleGetFunction(prologue): ") + hipGetErrorString(e));
    if (f_rows) e = hipModuleGetFunction(f_rows, *mod, ks.rows_name.c_str());
    if (e != hipSuccess) return fail(std::string("hipModuleGetFunction(rows): ") + hipGetErrorString(e));
    return 0;
}

long mmhip_filter_jit(mmhip_filter *f, int load_module) {
    auto t0 = std::chrono::steady_clock::now();
    if (jit_source(f->ks, f->code_object) != 0) return -1;
    for (mmhip_closure_kernel &ck : f->closures)
        if (jit_source(ck.ks, ck.code_object) != 0) return -1;
    if (load_module && !f->loaded) {
        if (load_kernels(f->ks, f->code_object, &f->mod, &f->f_pix, &f->f_pro, f->ks.row_values > 0 ? &f->f_rows : nullptr) != 0) return -1;
        for (mmhip_closure_kernel &ck : f->closures)
            if (!ck.loaded) {
                if (load_kernels(ck.ks, ck.code_object, &ck.mod, &ck.f_pix, &ck.f_pro) != 0) return -1;
                ck.loaded = true;
            }
        f->loaded = true;
    }
    f->jit_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return (long)f->code_object.size();
}

// The variants generated from the retained code (hipgen.h KernelOptions): the option that makes each one, and which
// filters have it.  None is for filters that call native filters or render closure images; `rows`: a per-row slice does
// not rule the variant out, and its kernel is mm_rows_clip.
struct GeneratedVariant {
    const char *name;
    void (*set)(KernelOptions &);
    bool rows;
    const char *refused;
};
static const GeneratedVariant generated_variants[VARIANT_COUNT] = {
    {nullptr, nullptr, true, nullptr},      // VARIANT_CLIP is not generated
    {"shutter", [](KernelOptions &ko) { ko.shutter = true; }, true, "it calls native filters or renders closure images"},
    {"sampled", [](KernelOptions &ko) { ko.sampled = true; }, false,
     "it calls native filters, renders closure images or has a per-row slice"},
    {"refine", [](KernelOptions &ko) { ko.sampled = ko.refine = true; }, false,
     "it calls native filters, renders closure images or has a per-row slice"},
};

// The text of one variant, made when it is first asked for: whatever else the filter has of text is a stored string and
// is not touched.  The clip variant is made from the main text (hipgen.cpp clip_kernel_source) and every filter has it;
// the others are generated from the retained code: null, with the message, for a filter that has none.  A variant whose
// generation failed stays empty, and is generated again when it is next asked for.
static const KernelSource *variant_source(mmhip_filter *f, int which) {
    KernelSource &ks = f->variants[which].ks;
    if (!ks.source.empty()) return &ks;
    const GeneratedVariant *g = &generated_variants[which];
    if (!g->set) {
        clip_kernel_source(f->ks, &ks.source, &ks.key);
        ks.prologue_name = "mm_prologue_clip";
        ks.rows_name = "mm_rows_clip";
        ks.pixel_name = "mm_pixels_clip";
        ks.wrapping_ints = f->ks.wrapping_ints;
        ks.row_values = f->ks.row_values;      // (of what the record describes this and the names alone are filled in)
        return &ks;
    }
    if (!f->ks.natives.empty() || !f->closures.empty() || (!g->rows && f->ks.row_values > 0)) {
        fail("filter `" + f->module.main->name + "' has no " + g->name + " variant: " + g->refused);
        return nullptr;
    }
    if (!f->code) { fail(std::string("filter has no ") + g->name + " variant: its code was not kept"); return nullptr; }
    try {
        KernelOptions ko = f->kopt;
        g->set(ko);
        ks = generate_hip(*f->code, ko);
    } catch (const std::exception &e) {
        ks = KernelSource();
        fail(e.what());
        return nullptr;
    }
    ks.prologue_name = "mm_prologue_clip";
    if (g->rows) ks.rows_name = "mm_rows_clip";
    return &ks;
}

static const char *variant_text(mmhip_filter *f, int which) {
    const KernelSource *ks = variant_source(f, which);
    return ks ? ks->source.c_str() : nullptr;
}

// hiprtc-compiles a variant and, where asked, loads its kernels: the code object's size, or -1.
static long jit_variant(mmhip_filter *f, int which, int load_module) {
    auto t0 = std::chrono::steady_clock::now();
    const KernelSource *ks = variant_source(f, which);
    ModuleVariant &v = f->variants[which];
    if (!ks || jit_source(*ks, v.code_object) != 0) return -1;
    if (load_module && !v.loaded) {
        if (load_kernels(*ks, v.code_object, &v.mod, &v.f_pix, &v.f_pro, ks->row_values > 0 ? &v.f_rows : nullptr) != 0) return -1;
        v.loaded = true;
    }
    f->jit_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return (long)v.code_object.size();
}

const char *mmhip_filter_clip_kernel_source(mmhip_filter *f) { return variant_text(f, VARIANT_CLIP); }
long mmhip_filter_jit_clip(mmhip_filter *f, int load_module) { return jit_variant(f, VARIANT_CLIP, load_module); }
const char *mmhip_filter_shutter_kernel_source(mmhip_filter *f) { return variant_text(f, VARIANT_SHUTTER); }
long mmhip_filter_jit_shutter(mmhip_filter *f, int load_module) { return jit_variant(f, VARIANT_SHUTTER, load_module); }
const char *mmhip_filter_sampled_kernel_source(mmhip_filter *f) { return variant_text(f, VARIANT_SAMPLED); }
long mmhip_filter_jit_sampled(mmhip_filter *f, int load_module) { return jit_variant(f, VARIANT_SAMPLED, load_module); }
const char *mmhip_filter_refine_kernel_source(mmhip_filter *f) { return variant_text(f, VARIANT_REFINE); }
long mmhip_filter_jit_refine(mmhip_filter *f, int load_module) { return jit_variant(f, VARIANT_REFINE, load_module); }

// ---------------------------------------------------------------------------
// invocation
// ---------------------------------------------------------------------------
mmhip_invocation *mmhip_invoke(mmhip_filter *f, int img_width, int img_height) {
    if (img_width <= 0 || img_height <= 0) { fail("image size must be positive"); return nullptr; }
    if (mmhip_filter_jit(f, 1) < 0) return nullptr;
    std::unique_ptr<mmhip_invocation> inv(new mmhip_invocation());
    inv->f = f;
    inv->img_w = inv->render_w = img_width;
    inv->img_h = inv->render_h = img_height;
    const auto &uvs = f->module.main->uservals;
    inv->uv.resize(std::max<size_t>(uvs.size(), 1));
    inv->image_slot_of_uv.assign(uvs.size(), -1);
    HImageDesc null_desc{};
    null_desc.kind = IMG_NULL;
    for (const UservalInfo &u : uvs) {   // defaults: userval.c:361-409
        HUserval &v = inv->uv[u.index];
        v.i = 0;
        switch (u.kind) {
            case UvKind::Int: v.i = u.idef; break;
            case UvKind::Float: v.f = u.fdef; break;
            case UvKind::Bool: v.i = u.bdef ? 1 : 0; break;
            case UvKind::Color: v.c = 0x000000ffu; break;   // opaque black
            case UvKind::Curve: {   // default curve: identity ramp (userval.c:282-311)
                v.i = (int)(inv->curves.size() / 1024);
                for (int i = 0; i < 1024; ++i) inv->curves.push_back((float)i / (float)(1024 - 1));
                break;
            }
            case UvKind::Gradient: {   // default gradient: opaque grey ramp (mathmap.c:356-361)
                v.i = (int)(inv->gradients.size() / 1024);
                for (int i = 0; i < 1024; ++i) {
                    float g = (float)i / (float)(1024 - 1);
                    uint32_t q = (uint32_t)(int)(g * 255.0) & 0xff;
                    inv->gradients.push_back((q << 24) | (q << 16) | (q << 8) | 255u);
                }
                break;
            }
            case UvKind::Image: {
                int slot = (int)inv->images.size();
                inv->image_slot_of_uv[u.index] = slot;
                inv->images.push_back(null_desc);
                v.image = slot;
                break;
            }
        }
    }
    inv->native_slot_base = (int)inv->images.size();
    inv->natives.resize(f->ks.natives.size());
    inv->images.resize(inv->images.size() + inv->natives.size(), null_desc);
    inv->closure_state.resize(f->closures.size());
    for (size_t c = 0; c < f->closures.size(); ++c) {      // the closure kernels' own native-filter results: slots of their own
        auto &st = inv->closure_state[c];
        st.native_slot_base = (int)inv->images.size();
        st.native_results.resize(f->closures[c].ks.natives.size());
        inv->images.resize(inv->images.size() + st.native_results.size(), null_desc);
    }
    if (inv->images.empty()) inv->images.push_back(null_desc);
    auto bail = [&](const char *what, hipError_t e) -> mmhip_invocation * {
        fail(std::string(what) + ": " + hipGetErrorString(e));
        return nullptr;
    };
    hipError_t e;
    if ((e = hipStreamCreate(&inv->stream.s)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = inv->d_uv.grow(inv->uv.size() * sizeof(HUserval))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = inv->d_images.grow(inv->images.size() * sizeof(HImageDesc))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = inv->d_curves.grow(inv->curves.size() * 4)) != hipSuccess) return bail("hipMalloc", e);
    if ((e = inv->d_gradients.grow(inv->gradients.size() * 4)) != hipSuccess) return bail("hipMalloc", e);
    const int xy_bytes = std::max(f->ks.xy_bytes, 256);
    if ((e = inv->launch.xy.grow(xy_bytes, DeviceBuffer::no_wait, true)) != hipSuccess) return bail("hipMalloc", e);
    return inv.release();
}

// Once the invocation's stream is idle the members go: the buffers are freed, the stream is destroyed last.
mmhip_invocation::~mmhip_invocation() {
    if (stream) (void)hipStreamSynchronize(stream);
    ws.release();
    for (auto &p : ev_pool) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
}

void mmhip_invocation_free(mmhip_invocation *inv) { delete inv; }

static const UservalInfo *uv_info(mmhip_invocation *inv, int index, UvKind kind) {
    const auto &uvs = inv->f->module.main->uservals;
    if (index < 0 || index >= (int)uvs.size()) { fail("user value index out of range"); return nullptr; }
    if (uvs[index].kind != kind) { fail("user value `" + uvs[index].name + "' has a different type"); return nullptr; }
    return &uvs[index];
}

int mmhip_set_int(mmhip_invocation *inv, int index, int value) {
    const UservalInfo *u = uv_info(inv, index, UvKind::Int);
    if (!u) return -1;
    inv->uv[index].i = value;
    inv->tables_dirty = true;
    return 0;
}

int mmhip_set_float(mmhip_invocation *inv, int index, float value) {
    const UservalInfo *u = uv_info(inv, index, UvKind::Float);
    if (!u) return -1;
    inv->uv[index].f = value;
    inv->tables_dirty = true;
    return 0;
}

int mmhip_set_bool(mmhip_invocation *inv, int index, int value) {
    const UservalInfo *u = uv_info(inv, index, UvKind::Bool);
    if (!u) return -1;
    inv->uv[index].i = value ? 1 : 0;
    inv->tables_dirty = true;
    return 0;
}

int mmhip_set_color(mmhip_invocation *inv, int index, float r, float g, float b, float a) {
    const UservalInfo *u = uv_info(inv, index, UvKind::Color);
    if (!u) return -1;
    auto q = [](float v) { v = v < 0 ? 0 : v > 1 ? 1 : v; return (uint32_t)(v * 255.0); };
    inv->uv[index].c = (q(r) << 24) | (q(g) << 16) | (q(b) << 8) | q(a);
    inv->tables_dirty = true;
    return 0;
}

// -Dname=value (mathmap_cmdline.c:756-796; images are bound by the caller)
int mmhip_set_by_name(mmhip_invocation *inv, const char *name, const char *value) {
    for (const UservalInfo &u : inv->f->module.main->uservals) {
        if (u.name != name) continue;
        switch (u.kind) {
            case UvKind::Int: return mmhip_set_int(inv, u.index, atoi(value));
            case UvKind::Float: return mmhip_set_float(inv, u.index, (float)atof(value));
            case UvKind::Bool: return mmhip_set_bool(inv, u.index, atoi(value));
            default: return fail(std::string("user value `") + name + "' cannot be set from a string");
        }
    }
    return fail(std::string("filter has no user value `") + name + "'");
}

// `data` holds num_frames frames of w x h texels, one after the other; scale and middle are those of one frame
static void fill_drawable_desc(HImageDesc &d, const void *data, int w, int h, int num_frames) {
    d.data = data;
    d.w = w;
    d.h = h;
    d.kind = IMG_DRAWABLE;
    d.num_frames = num_frames;
    d.scale_x = (float)((w - 1) / 2.0);    // userval.c:272-276
    d.scale_y = (float)((h - 1) / 2.0);
    d.middle_x = 1.0f;
    d.middle_y = 1.0f;
    d.ax = d.bx = d.ay = d.by = 0.f;
}

// A native float map (the result of a native filter, or a closure image rendered for one) as the kernels read it.
HImageDesc floatmap_desc(const void *data, int w, int h) {
    HImageDesc d{};
    d.data = data;
    d.w = w;
    d.h = h;
    d.kind = IMG_FLOATMAP;
    d.num_frames = 1;
    d.ax = d.bx = (float)((float)(w - 1) / 2.0);     // floatmap.c:39-41
    d.ay = d.by = (float)((float)(h - 1) / 2.0);
    d.ay *= -1.0f;
    return d;
}

// An input image was bound or unbound: the tables go up again, and every native result is stale.
static void input_changed(mmhip_invocation *inv) {
    inv->tables_dirty = true;
    ++inv->input_generation;
}

// Bytes of num_frames packed frames, or false where the count is not a size (a negative extent, overflow) or the
// sequence has more rows than an int counts.
static bool sequence_bytes(int width, int height, int num_frames, size_t &bytes) {
    if (width < 0 || height < 0 || num_frames < 1) return false;
    size_t texels = 0;
    // (the generic fetch addresses row frame * height + y of the sequence in an int: mm_get_pixel_cold)
    if ((uint64_t)height * (uint64_t)num_frames > (uint64_t)INT32_MAX) return false;
    return !__builtin_mul_overflow((size_t)width, (size_t)height, &texels) && !__builtin_mul_overflow(texels, (size_t)num_frames, &texels) &&
           !__builtin_mul_overflow(texels, (size_t)4, &bytes) && bytes <= (size_t)PTRDIFF_MAX;
}

// The upload bound to `slot`, if it was ours, goes once nothing in flight reads it.
static void release_owned_image(mmhip_invocation *inv, int slot) {
    const void *old = inv->images[slot].data;
    for (auto it = inv->owned.begin(); it != inv->owned.end(); ++it)
        if (it->get() == old) {
            (void)hipDeviceSynchronize();     // renders may have been queued on caller streams
            inv->owned.erase(it);
            return;
        }
}

int mmhip_set_image_sequence_device(mmhip_invocation *inv, int index, const void *device_rgba32, int width, int height, int num_frames) {
    // (the arguments first: what is wrong with them does not depend on the invocation)
    if (num_frames < 1) return fail("num_frames must be at least 1");
    size_t bytes = 0;
    if (!sequence_bytes(width, height, num_frames, bytes)) return fail("image sequence: the size overflows (fewer than 2^31 rows in all, and a byte count that fits)");
    const UservalInfo *u = uv_info(inv, index, UvKind::Image);
    if (!u) return -1;
    int slot = inv->image_slot_of_uv[index];
    if (inv->images[slot].kind == IMG_DEEP && inv->images[slot].data != device_rgba32) release_owned_image(inv, slot);      // a float32 upload of ours
    fill_drawable_desc(inv->images[slot], device_rgba32, width, height, num_frames);
    input_changed(inv);
    return 0;
}

int mmhip_set_image_device(mmhip_invocation *inv, int index, const void *device_rgba32, int width, int height) {
    return mmhip_set_image_sequence_device(inv, index, device_rgba32, width, height, 1);
}

void mmhip_unbind_image(mmhip_invocation *inv, const void *data) {
    for (HImageDesc &img : inv->images)
        if (img.data == data) {
            img.kind = IMG_NULL;
            img.data = nullptr;
            input_changed(inv);
        }
}

int mmhip_set_image_sequence_host(mmhip_invocation *inv, int index, const uint8_t *pixels, int width, int height, int channels,
                                  int num_frames) {
    if (channels != 3 && channels != 4) return fail("channels must be 3 or 4");
    if (num_frames < 1) return fail("num_frames must be at least 1");
    size_t bytes = 0;
    if (!sequence_bytes(width, height, num_frames, bytes)) return fail("image sequence: the size overflows (fewer than 2^31 rows in all, and a byte count that fits)");
    if (!uv_info(inv, index, UvKind::Image)) return -1;
    const size_t n = (size_t)width * height;
    // one frame at a time through one staging buffer: the frames land one after the other
    std::vector<uint32_t> packed;
    try { packed.resize(n); } catch (const std::bad_alloc &) { return fail("image sequence: out of host memory"); }
    DeviceBuffer d;
    HIP_TRY(d.grow(bytes));
    for (int k = 0; k < num_frames; ++k) {
        const uint8_t *frame = pixels + (size_t)k * n * channels;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t *p = frame + i * channels;
            uint32_t a = channels == 4 ? p[3] : 255u;
            packed[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | a;
        }
        HIP_TRY(hipMemcpy((char *)d.get() + (size_t)k * n * 4, packed.data(), n * 4, hipMemcpyHostToDevice));
    }
    // the upload this one replaces (if it was ours) is freed once nothing in flight reads it
    const void *old = inv->images[inv->image_slot_of_uv[index]].data;
    for (auto it = inv->owned.begin(); it != inv->owned.end(); ++it)
        if (it->get() == old) {
            (void)hipDeviceSynchronize();     // renders may have been queued on caller streams
            inv->owned.erase(it);
            break;
        }
    const void *dev = d.get();
    inv->owned.push_back(std::move(d));
    return mmhip_set_image_sequence_device(inv, index, dev, width, height, num_frames);
}

// ---- float32 drawables (mmhip_options.deep_inputs; the semantics are stated in include/mmhip.h) ----

// What is wrong with the arguments of a deep-image setter, checked before the invocation is looked at and before anything
// is allocated or bound; `bytes` becomes the size of the sequence (16 bytes a texel).
static int check_deep_sequence(const std::string &who, const void *p, bool device, int width, int height, int num_frames, size_t *bytes) {
    if (width < 1 || height < 1) return fail(who + "width and height must be at least 1, not " + std::to_string(width) + " x " + std::to_string(height));
    if (num_frames < 1) return fail(who + "num_frames must be at least 1");
    if (!p) return fail(who + "the pixels are a null pointer");
    if (device && ((uintptr_t)p & 15u) != 0) return fail(who + "the device pointer is not 16-byte aligned (float4 texels)");
    size_t words = 0;
    // (sequence_bytes counts 4 bytes a texel and applies the row rule of the generic fetch, which mm_get_pixel_deep shares)
    if (!sequence_bytes(width, height, num_frames, words) || __builtin_mul_overflow(words, (size_t)4, bytes) || *bytes > (size_t)PTRDIFF_MAX)
        return fail(who + "the size overflows (fewer than 2^31 rows in all, and a byte count that fits)");
    return 0;
}

// ... and with the invocation: its filter's kernels must know the kind
static int check_deep_filter(const std::string &who, const mmhip_invocation *inv) {
    if (!inv) return fail(who + "no invocation");
    if (!inv->f->kopt.deep_inputs)
        return fail(who + "filter `" + inv->f->module.main->name + "' was not compiled with deep_inputs (mmhip_options.deep_inputs = 1)");
    return 0;
}

static void bind_deep_image(mmhip_invocation *inv, int slot, const void *data, int width, int height, int num_frames) {
    fill_drawable_desc(inv->images[slot], data, width, height, num_frames);
    inv->images[slot].kind = IMG_DEEP;
    input_changed(inv);
}

int mmhip_set_image_sequence_float_device(mmhip_invocation *inv, int index, const void *device_float4, int width, int height, int num_frames) {
    const std::string who = "set_image_sequence_float_device: ";
    size_t bytes = 0;
    if (check_deep_sequence(who, device_float4, true, width, height, num_frames, &bytes) != 0 || check_deep_filter(who, inv) != 0) return -1;
    if (!uv_info(inv, index, UvKind::Image)) return -1;
    const int slot = inv->image_slot_of_uv[index];
    if (inv->images[slot].data != device_float4) release_owned_image(inv, slot);
    bind_deep_image(inv, slot, device_float4, width, height, num_frames);
    return 0;
}

int mmhip_set_image_sequence_float_host(mmhip_invocation *inv, int index, const float *pixels, int width, int height, int channels, int num_frames) {
    const std::string who = "set_image_sequence_float_host: ";
    if (channels != 3 && channels != 4) return fail(who + "channels must be 3 or 4, not " + std::to_string(channels));
    size_t bytes = 0;
    if (check_deep_sequence(who, pixels, false, width, height, num_frames, &bytes) != 0 || check_deep_filter(who, inv) != 0) return -1;
    if (!uv_info(inv, index, UvKind::Image)) return -1;
    const size_t n = (size_t)width * height;
    DeviceBuffer d;
    HIP_TRY(d.grow(bytes));
    if (channels == 4) HIP_TRY(hipMemcpy(d.get(), pixels, bytes, hipMemcpyHostToDevice));
    else {
        // one frame at a time through one staging buffer, alpha 1.0f: the frames land one after the other
        std::vector<float> texels;
        try { texels.resize(n * 4); } catch (const std::bad_alloc &) { return fail(who + "out of host memory"); }
        for (int k = 0; k < num_frames; ++k) {
            const float *frame = pixels + (size_t)k * n * 3;
            for (size_t i = 0; i < n; ++i) {
                texels[i * 4 + 0] = frame[i * 3 + 0];
                texels[i * 4 + 1] = frame[i * 3 + 1];
                texels[i * 4 + 2] = frame[i * 3 + 2];
                texels[i * 4 + 3] = 1.0f;
            }
            HIP_TRY(hipMemcpy(d.get<char>() + (size_t)k * n * 16, texels.data(), n * 16, hipMemcpyHostToDevice));
        }
    }
    const int slot = inv->image_slot_of_uv[index];
    release_owned_image(inv, slot);
    const void *dev = d.get();
    inv->owned.push_back(std::move(d));
    bind_deep_image(inv, slot, dev, width, height, num_frames);
    return 0;
}

// The staged upload of planar Y'CbCr 4:2:0 payloads, of either depth: frame i's frame_bytes at payloads + i * frame_stride
// go up as they are, in groups of at most 65 535 frames through a staging buffer of at most MMHIP_CLIP_YUV_IN_BYTES (256
// MiB where it is not set), and convert(staged, n, to, stream) expands each group of n frames to its place in `landed`,
// landed_bytes a frame.  *groups counts them.  The stream is waited for before a group overwrites what the launch before
// it reads, and after the last.
template <class Convert>
static int upload_yuv_groups(mmhip_invocation *inv, const void *payloads, int64_t frame_stride, int64_t frame_bytes, char *landed, int64_t landed_bytes,
                             int num_frames, int *groups, Convert convert) {
    const char *text = getenv("MMHIP_CLIP_YUV_IN_BYTES");
    long long budget = text ? atoll(text) : 0;
    if (budget <= 0) budget = (long long)256 << 20;
    const int per_group = (int)std::max<long long>(1, std::min<long long>(std::min(num_frames, 65535), budget / frame_bytes));
    DeviceBuffer staging;
    HIP_TRY(staging.grow((size_t)per_group * (size_t)frame_bytes));
    hipStream_t s = (hipStream_t)inv->stream;
    *groups = 0;
    for (int g0 = 0; g0 < num_frames; g0 += per_group) {
        const int n = std::min(per_group, num_frames - g0);
        if (g0) HIP_TRY(hipStreamSynchronize(s));      // the launch before this one reads the staging buffer
        const char *from = (const char *)payloads + (size_t)g0 * (size_t)frame_stride;
        if (frame_stride == frame_bytes) HIP_TRY(hipMemcpy(staging.get(), from, (size_t)n * (size_t)frame_bytes, hipMemcpyHostToDevice));
        else
            for (int k = 0; k < n; ++k)
                HIP_TRY(hipMemcpy(staging.get<char>() + (size_t)k * (size_t)frame_bytes, from + (size_t)k * (size_t)frame_stride, (size_t)frame_bytes,
                                  hipMemcpyHostToDevice));
        if (convert(staging.get(), n, landed + (size_t)g0 * (size_t)landed_bytes, s) != 0) return -1;
        ++*groups;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// Planar Y'CbCr 4:2:0 payloads as a sequence: they go up as they are, in groups through a staging buffer of at most
// MMHIP_CLIP_YUV_IN_BYTES, and k_yuv420_to_rgba_clip expands every group into the owned sequence.
static int set_image_sequence_yuv420_host(const std::string &name, bool sited, mmhip_invocation *inv, int index, const uint8_t *yuv, int64_t frame_stride, int width,
                                          int height, int num_frames, int matrix, int range, int chroma, int siting) {
    const std::string who = name + ": ";
    const char *converter = sited ? "clip_from_yuv420_sited" : "clip_from_yuv420";
    if (width < 1 || height < 1) return fail(who + "width and height must be at least 1, not " + std::to_string(width) + " x " + std::to_string(height));
    if (num_frames < 1) return fail("num_frames must be at least 1");
    size_t bytes = 0;
    if (!sequence_bytes(width, height, num_frames, bytes)) return fail("image sequence: the size overflows (fewer than 2^31 rows in all, and a byte count that fits)");
    if (!yuv) return fail(who + "no payloads");
    const int64_t frame_bytes = mmhip_yuv420_frame_bytes(width, height), words_bytes = (int64_t)width * height * 4;
    if (frame_stride < frame_bytes)
        return fail(who + "frame_stride " + std::to_string(frame_stride) + " is smaller than one frame (" + std::to_string(frame_bytes) + " bytes)");
    std::string err;
    // (the converter's own refusals before anything is allocated: the pointers are placeholders)
    const YuvInJob job = {converter, yuv, frame_bytes, width, height, 1, matrix, range, chroma, siting, (void *)yuv, words_bytes};
    if (check_yuv420_to_rgba_clip(job, &err) != 0) return fail(err);
    if (!uv_info(inv, index, UvKind::Image)) return -1;
    DeviceBuffer d;
    HIP_TRY(d.grow(bytes));
    if (upload_yuv_groups(inv, yuv, frame_stride, frame_bytes, d.get<char>(), words_bytes, num_frames, &inv->clip_yuv_input_groups,
                          [&](const void *staged, int n, void *to, hipStream_t s) {
                              return sited ? mmhip_clip_from_yuv420_sited(inv, staged, frame_bytes, width, height, n, matrix, range, chroma, siting, to, words_bytes, s)
                                           : mmhip_clip_from_yuv420(inv, staged, frame_bytes, width, height, n, matrix, range, chroma, to, words_bytes, s);
                          }) != 0)
        return -1;
    // the upload this one replaces (if it was ours) is freed once nothing in flight reads it
    const void *old = inv->images[inv->image_slot_of_uv[index]].data;
    for (auto it = inv->owned.begin(); it != inv->owned.end(); ++it)
        if (it->get() == old) {
            (void)hipDeviceSynchronize();     // renders may have been queued on caller streams
            inv->owned.erase(it);
            break;
        }
    const void *dev = d.get();
    inv->owned.push_back(std::move(d));
    return mmhip_set_image_sequence_device(inv, index, dev, width, height, num_frames);
}

int mmhip_set_image_sequence_yuv420_host(mmhip_invocation *inv, int index, const uint8_t *yuv, int64_t frame_stride, int width, int height,
                                         int num_frames, int matrix, int range, int chroma) {
    return set_image_sequence_yuv420_host("set_image_sequence_yuv420_host", false, inv, index, yuv, frame_stride, width, height, num_frames, matrix, range, chroma,
                                          MMHIP_YUV_SITING_CENTER);
}

int mmhip_set_image_sequence_yuv420_host_sited(mmhip_invocation *inv, int index, const uint8_t *yuv, int64_t frame_stride, int width, int height,
                                               int num_frames, int matrix, int range, int chroma, int siting) {
    return set_image_sequence_yuv420_host("set_image_sequence_yuv420_host_sited", true, inv, index, yuv, frame_stride, width, height, num_frames, matrix, range,
                                          chroma, siting);
}

// The same for payloads of 16-bit samples and a deep drawable: 3 bytes a pixel go up, k_yuv420p10_to_float_clip expands
// every group into the owned sequence of float4 texels.
static int set_image_sequence_yuv420p10_host(const std::string &name, bool sited, mmhip_invocation *inv, int index, const uint16_t *yuv, int64_t frame_stride,
                                             int width, int height, int num_frames, int matrix, int range, int chroma, int siting) {
    const std::string who = name + ": ";
    const char *converter = sited ? "clip_from_yuv420p10_sited" : "clip_from_yuv420p10";
    size_t bytes = 0;
    if (check_deep_sequence(who, yuv, false, width, height, num_frames, &bytes) != 0 || check_deep_filter(who, inv) != 0) return -1;
    const int64_t frame_bytes = mmhip_yuv420p10_frame_bytes(width, height), texel_bytes = (int64_t)width * height * 16;
    if (frame_stride % 2 != 0) return fail(who + "frame_stride " + std::to_string(frame_stride) + " is odd (the samples are 16-bit)");
    if (frame_stride < frame_bytes)
        return fail(who + "frame_stride " + std::to_string(frame_stride) + " is smaller than one frame (" + std::to_string(frame_bytes) + " bytes)");
    std::string err;
    // (the converter's own refusals before anything is allocated: the pointers are placeholders)
    const YuvInJob job = {converter, (const void *)16, frame_bytes, width, height, 1, matrix, range, chroma, siting, (void *)16, texel_bytes};
    if (check_yuv420p10_to_float_clip(job, &err) != 0) return fail(err);
    if (!uv_info(inv, index, UvKind::Image)) return -1;
    DeviceBuffer d;
    HIP_TRY(d.grow(bytes));
    if (upload_yuv_groups(inv, yuv, frame_stride, frame_bytes, d.get<char>(), texel_bytes, num_frames, &inv->clip_yuv10_input_groups,
                          [&](const void *staged, int n, void *to, hipStream_t s) {
                              return sited ? mmhip_clip_from_yuv420p10_sited(inv, staged, frame_bytes, width, height, n, matrix, range, chroma, siting, to, texel_bytes, s)
                                           : mmhip_clip_from_yuv420p10(inv, staged, frame_bytes, width, height, n, matrix, range, chroma, to, texel_bytes, s);
                          }) != 0)
        return -1;
    const int slot = inv->image_slot_of_uv[index];
    release_owned_image(inv, slot);
    const void *dev = d.get();
    inv->owned.push_back(std::move(d));
    bind_deep_image(inv, slot, dev, width, height, num_frames);
    return 0;
}

int mmhip_set_image_sequence_yuv420p10_host(mmhip_invocation *inv, int index, const uint16_t *yuv, int64_t frame_stride, int width, int height,
                                            int num_frames, int matrix, int range, int chroma) {
    return set_image_sequence_yuv420p10_host("set_image_sequence_yuv420p10_host", false, inv, index, yuv, frame_stride, width, height, num_frames, matrix, range,
                                             chroma, MMHIP_YUV_SITING_CENTER);
}

int mmhip_set_image_sequence_yuv420p10_host_sited(mmhip_invocation *inv, int index, const uint16_t *yuv, int64_t frame_stride, int width, int height,
                                                  int num_frames, int matrix, int range, int chroma, int siting) {
    return set_image_sequence_yuv420p10_host("set_image_sequence_yuv420p10_host_sited", true, inv, index, yuv, frame_stride, width, height, num_frames, matrix,
                                             range, chroma, siting);
}

int mmhip_set_image_host(mmhip_invocation *inv, int index, const uint8_t *pixels, int width, int height, int channels) {
    return mmhip_set_image_sequence_host(inv, index, pixels, width, height, channels, 1);
}

int mmhip_set_curve(mmhip_invocation *inv, int index, const float *values1024) {
    if (!uv_info(inv, index, UvKind::Curve)) return -1;
    float *dst = &inv->curves[(size_t)inv->uv[index].i * 1024];
    if (memcmp(dst, values1024, 1024 * sizeof(float)) == 0) return 0;     // unchanged: no re-upload
    memcpy(dst, values1024, 1024 * sizeof(float));
    inv->tables_dirty = true;
    return 0;
}

int mmhip_set_gradient(mmhip_invocation *inv, int index, const uint32_t *rgba1024) {
    if (!uv_info(inv, index, UvKind::Gradient)) return -1;
    uint32_t *dst = &inv->gradients[(size_t)inv->uv[index].i * 1024];
    if (memcmp(dst, rgba1024, 1024 * sizeof(uint32_t)) == 0) return 0;
    memcpy(dst, rgba1024, 1024 * sizeof(uint32_t));
    inv->tables_dirty = true;
    return 0;
}

// Row-striped rendering of filters with native-filter calls (one stripe per GPU): with a margin
// >= 0 a render of rows [a, b) of the full frame lets the native filters fill only rows
// [a - margin, b + margin) of their maps (plus whatever halo the filter itself needs).  The caller
// asserts that the filter samples a native map no further than `margin` rows from the output row
// (0 for `blurred(xy)`).  -1 (default): always the whole map, like the reference.
int mmhip_set_native_row_margin(mmhip_invocation *inv, int margin) {
    inv->native_row_margin = margin;
    return 0;
}

int mmhip_set_native_input_frame(mmhip_invocation *inv, int mode) {
    if (mode != MMHIP_NATIVE_FRAME_ZERO && mode != MMHIP_NATIVE_FRAME_CURRENT)
        return fail("native input frame: mode " + std::to_string(mode) + " is neither MMHIP_NATIVE_FRAME_ZERO (0) nor MMHIP_NATIVE_FRAME_CURRENT (1)");
    if (inv->native_input_frame != mode) ++inv->input_generation;      // what the native results were computed from changes
    inv->native_input_frame = mode;
    return 0;
}

int mmhip_set_edge_colors(mmhip_invocation *inv, uint32_t cx, uint32_t cy) {
    // render(in) keeps the drawable's resize wrapper, so k_render_drawable samples beyond the edges with these colours
    // (set_native_env): a change of either makes the native results stale; the values they have leave the memo alone
    if (inv->edge_color_x != cx || inv->edge_color_y != cy) ++inv->input_generation;
    inv->edge_color_x = cx;
    inv->edge_color_y = cy;
    return 0;
}

int mmhip_set_render_size(mmhip_invocation *inv, int rw, int rh) {
    inv->render_w = rw;
    inv->render_h = rh;
    return 0;
}

int mmhip_set_sampling_offset(mmhip_invocation *inv, float ox, float oy) {
    inv->sampling_offset_x = ox;
    inv->sampling_offset_y = oy;
    return 0;
}

int mmhip_enable_timing(mmhip_invocation *inv, int on) {
    inv->timing = on != 0;
    inv->ws.timing = on != 0;
    return 0;
}

// Durations (ms) of the native filters' own kernels (gaussian_blur: its four scan kernels) launched since the last
// drain, in launch order; names[i * 64 ...] receives the kernel's label.  Waits for the last of them.
int mmhip_drain_native_kernel_ms(mmhip_invocation *inv, char *names, double *out_ms, int cap) {
    auto &tm = inv->ws.timed;
    if (!tm.empty() && hipEventSynchronize(tm.back().b) != hipSuccess) return fail("event sync failed");
    int n = 0;
    for (auto &t : tm) {
        float ms = 0;
        if (n < cap && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
            snprintf(names + (size_t)n * 64, 64, "%s", t.name);
            out_ms[n++] = ms;
        }
        inv->ws.timed_free.push_back({t.a, t.b});
    }
    tm.clear();
    return n;
}

// The next event pair for a timed launch (grown on demand, wraps after 4096 pending launches).
static int next_event_pair(mmhip_invocation *inv) {
    if (inv->ev_used == inv->ev_pool.size()) {
        if (inv->ev_pool.size() >= 4096) inv->ev_used = 0;
        else {
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a));
            HIP_TRY(hipEventCreate(&b));
            inv->ev_pool.push_back({a, b});
        }
    }
    inv->ev0 = inv->ev_pool[inv->ev_used].first;
    inv->ev1 = inv->ev_pool[inv->ev_used].second;
    ++inv->ev_used;
    return 0;
}

// The pixel launch of a render between the event pair of a timed invocation.  f_pix null: a native filter has written
// the pixels (run_natives) and nothing is launched; the pair is recorded all the same.
int timed_pixel_launch(mmhip_invocation *inv, hipFunction_t f_pix, unsigned grid_x, unsigned grid_y, void **params, hipStream_t s) {
    if (inv->timing) {
        if (next_event_pair(inv) != 0) return -1;
        HIP_TRY(hipEventRecord(inv->ev0, s));
    }
    if (f_pix) HIP_TRY(hipModuleLaunchKernel(f_pix, grid_x, grid_y, 1, 256, 1, 1, 0, s, params, nullptr));
    if (inv->timing) {
        HIP_TRY(hipEventRecord(inv->ev1, s));
        inv->ev_valid = true;
    }
    return 0;
}

// Durations (ms) of the pixel kernel of every timed launch since the last drain, oldest first;
// waits for the last of them.  Returns how many were written (at most `cap`).
long mmhip_direct_native_launches(mmhip_invocation *inv) { return inv->direct_native_launches; }
long mmhip_tolerance_blur_launches(mmhip_invocation *inv) { return inv->tolerance_blur_launches; }
long mmhip_prologue_launches(mmhip_invocation *inv) { return inv->prologue_launches; }
long mmhip_native_memo_hits(mmhip_invocation *inv) { return inv->native_memo_hits; }

int mmhip_drain_kernel_ms(mmhip_invocation *inv, double *out_ms, int cap) {
    int n = 0;
    if (inv->ev_used > 0 && hipEventSynchronize(inv->ev_pool[inv->ev_used - 1].second) != hipSuccess) return fail("event sync failed");
    for (size_t i = 0; i < inv->ev_used && n < cap; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, inv->ev_pool[i].first, inv->ev_pool[i].second) != hipSuccess) return fail("event elapsed failed");
        out_ms[n++] = ms;
    }
    inv->ev_used = 0;
    inv->ev_valid = false;
    return n;
}

double mmhip_last_kernel_ms(mmhip_invocation *inv) {
    if (!inv->ev_valid) return -1.0;
    if (hipEventSynchronize(inv->ev1) != hipSuccess) return -1.0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, inv->ev0, inv->ev1) != hipSuccess) return -1.0;
    return ms;
}

// the image table to the device, once nothing in flight on `s` still reads the old one
static int upload_image_table(mmhip_invocation *inv, hipStream_t s) {
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(inv->d_images.get(), inv->images.data(), inv->images.size() * sizeof(HImageDesc), hipMemcpyHostToDevice));
    return 0;
}

int upload_tables(mmhip_invocation *inv, hipStream_t s) {
    if (!inv->tables_dirty) return 0;
    if (upload_image_table(inv, s) != 0) return -1;
    HIP_TRY(hipMemcpy(inv->d_uv.get(), inv->uv.data(), inv->uv.size() * sizeof(HUserval), hipMemcpyHostToDevice));
    if (inv->d_curves) HIP_TRY(hipMemcpy(inv->d_curves.get(), inv->curves.data(), inv->curves.size() * 4, hipMemcpyHostToDevice));
    if (inv->d_gradients) HIP_TRY(hipMemcpy(inv->d_gradients.get(), inv->gradients.data(), inv->gradients.size() * 4, hipMemcpyHostToDevice));
    inv->tables_dirty = false;
    ++inv->table_generation;
    return 0;
}

// rows per work-item for that many workgroups at one row each: enough workgroups must remain to fill 256 CUs several times over
static int rows_per_item(long wgs) { return wgs >= 262144 ? 16 : wgs >= 131072 ? 8 : wgs >= 32768 ? 4 : wgs >= 8192 ? 2 : 1; }

// the launch at `ppt` rows per work-item, or what MMHIP_PPT and the kernel's shape make of them
static void set_rows_per_item(LaunchGeometry &g, const KernelSource &ks, int num_rows, int ppt) {
    if (const char *e = getenv("MMHIP_PPT")) ppt = std::max(1, atoi(e));
    if (ks.single_pixel) ppt = 1;
    const int u = std::max(1, ks.unroll);          // the kernel steps MM_UNROLL rows at a time
    g.ppt = (ppt + u - 1) / u * u;
    g.tiles_y = (num_rows + ks.tile_h * g.ppt - 1) / (ks.tile_h * g.ppt);
    g.nwg = (long)g.tiles_x * g.tiles_y;
    g.tiles_magic = tile_division_magic(g.tiles_x, g.nwg);
}

static LaunchGeometry launch_geometry(const KernelSource &ks, int region_w, int num_rows) {
    LaunchGeometry g;
    g.tiles_x = (region_w + ks.tile_w - 1) / ks.tile_w;
    g.wg1 = (long)g.tiles_x * ((num_rows + ks.tile_h - 1) / ks.tile_h);
    set_rows_per_item(g, ks, num_rows, rows_per_item(g.wg1));
    return g;
}

// The geometry of one frame of a clip launch (mm_pixels_clip over `frames` frames at once): the rows-per-item choice is
// made from the workgroups of the whole batch -- a 1920x1080 frame alone is too small to share a work-item's start-up
// cost between rows, 120 of them are not -- but a work-item's rows stay rows of its own frame: no more of them than the
// frame has tile rows (or than the frame alone would get).  With frames = 1 this is launch_geometry.
LaunchGeometry clip_launch_geometry(const KernelSource &ks, int region_w, int num_rows, int frames) {
    LaunchGeometry g = launch_geometry(ks, region_w, num_rows);
    const int tile_rows = (num_rows + ks.tile_h - 1) / ks.tile_h;
    set_rows_per_item(g, ks, num_rows, std::min(rows_per_item(g.wg1 * std::max(frames, 1)), std::max(rows_per_item(g.wg1), tile_rows)));
    return g;
}

// How a clip of `frames` frames is cut into launches: gridDim.x is the frame's workgroups rounded up to a multiple of 8
// (a workgroup's XCD is then blockIdx.x & 7 in every grid row), gridDim.y at most 65 535 frames, the grid below 2^31
// work-items, and MMHIP_CLIP_MAX_FRAMES (read once) lowers the frames per launch.  max_frames 0: one frame alone is too
// large for the grid, and the clip is rendered frame by frame.
ClipPlan clip_plan(const LaunchGeometry &g) {
    static const int env_cap = [] {
        const char *e = getenv("MMHIP_CLIP_MAX_FRAMES");
        return e && atoi(e) > 0 ? atoi(e) : 65535;
    }();
    ClipPlan p;
    p.grid_x = (g.nwg + 7) / 8 * 8;
    const long by_items = ((1L << 23) - 1) / p.grid_x;      // grid_x * frames * 256 < 2^31
    p.max_grid_rows = std::min(65535, env_cap);
    p.max_rows_by_items = by_items;
    p.max_frames = (int)std::min<long>(p.max_grid_rows, by_items);
    return p;
}

LaunchGeometry single_pixel_launch_geometry(const KernelSource &ks, int region_w, int num_rows) {
    KernelSource single;
    single.tile_w = ks.tile_w;
    single.tile_h = ks.tile_h;
    single.unroll = 1;
    single.single_pixel = true;
    return launch_geometry(single, region_w, num_rows);
}

static int geometry_out(const KernelSource &ks, int region_w, int num_rows, int64_t *out, int clip_frames = 0) {
    if (region_w < 1 || num_rows < 1) return fail("launch geometry: empty region");
    const LaunchGeometry g = clip_frames > 0 ? clip_launch_geometry(ks, region_w, num_rows, clip_frames) : launch_geometry(ks, region_w, num_rows);
    // the kernel's XCD order 2 swizzles the first `full' workgroups: whole rounds of 8 runs of 2^m tiles (hipgen.cpp)
    int m = 0;
    for (unsigned v = (unsigned)(g.tiles_x > 1 ? g.tiles_x - 1 : 1); v; v >>= 1) ++m;
    const int64_t v[MMHIP_GEOMETRY_FIELDS] = {g.tiles_x, g.tiles_y, g.wg1, g.nwg, g.ppt, ks.tile_w, ks.tile_h, ks.unroll,
                                              ks.pair_mode, ks.single_pixel, ks.xcd_order, (int64_t)g.tiles_magic,
                                              (g.nwg >> (m + 3)) << (m + 3)};
    memcpy(out, v, sizeof v);
    return 0;
}

int mmhip_filter_launch_geometry(const mmhip_filter *f, int region_w, int num_rows, int64_t *out) {
    return geometry_out(f->ks, region_w, num_rows, out);
}

int mmhip_filter_clip_launch_geometry(const mmhip_filter *f, int region_w, int num_rows, int frames, int64_t *out) {
    if (frames < 1) return fail("clip launch geometry: num_frames must be at least 1");
    return geometry_out(f->ks, region_w, num_rows, out, frames);
}

int mmhip_filter_clip_batch_plan(const mmhip_filter *f, int region_w, int num_rows, int frames, int64_t *out) {
    if (frames < 1) return fail("clip batch plan: num_frames must be at least 1");
    if (region_w < 1 || num_rows < 1) return fail("clip batch plan: empty region");
    const bool batched = f->ks.natives.empty() && f->closures.empty();
    const ClipPlan p = clip_plan(clip_launch_geometry(f->ks, region_w, num_rows, frames));
    const int64_t per = batched ? p.max_frames : 0;
    const int64_t v[MMHIP_CLIP_PLAN_FIELDS] = {p.grid_x, per, per ? (frames + per - 1) / per : 0, !f->ks.prologue_uses_time};
    memcpy(out, v, sizeof v);
    return 0;
}

int mmhip_filter_num_closures(const mmhip_filter *f) { return (int)f->closures.size(); }

int mmhip_filter_closure_launch_geometry(const mmhip_filter *f, int closure, int width, int height, int64_t *out) {
    if (closure < 0 || closure >= (int)f->closures.size()) return fail("launch geometry: no such closure image");
    return geometry_out(f->closures[closure].ks, width, height, out);
}

// The buffers of a launch of `ks` over `num_rows` rows of a `region_w`-wide region, grown on demand (stream order protects
// re-use): coordinate tables, with `rows` the per-row values, and the frame constants (zero-filled when new).
int grow_launch_buffers(LaunchBuffers &b, const KernelSource &ks, int region_w, int num_rows, bool rows, hipStream_t s) {
    auto wait = [s] { return hipStreamSynchronize(s); };
    HIP_TRY(b.xtab.grow((size_t)region_w * sizeof(float), wait));
    HIP_TRY(b.ytab.grow((size_t)num_rows * sizeof(float), wait));
    if (rows) HIP_TRY(b.rowtab.grow((size_t)ks.row_values * num_rows * sizeof(float), wait));
    HIP_TRY(b.xy.grow(std::max(ks.xy_bytes, 256), wait, true));
    return 0;
}

// render_image's closure branch (builtins.c:273-298): closure image #cid of the filter rendered over the
// whole frame into a float map -- calc_lines(slice 0,0,w,h; first_row 0, last_row h; floatmap = 1) on a
// frame made by invocation_new_frame(invocation, image, 0, 0.0): frame 0, t = 0, sampling offsets 0.
// The native-filter calls the prologue recorded in `host' (a copy of the frame-constant buffer), in the order they
// were made: entry k of ks.natives (a call site outside loops, or the n-th dynamic entry of the in-loop sites) and its
// record.  The record's `pad' is the call's number within the frame (mm_native_call in hipgen.cpp).
int recorded_calls(const KernelSource &ks, const char *host, std::vector<RecordedCall> *calls) {
    calls->clear();
    if (ks.natives.empty()) return 0;
    int ctr[4];
    memcpy(ctr, host + ks.native_ctr_offset, sizeof ctr);
    if (ctr[2])
        return fail("native filters are called more than " + std::to_string((int)MM_NATIVE_DYN_CALLS) +
                    " times from inside a loop of the frame-constant code: not supported");
    for (size_t k = 0; k < ks.natives.size(); ++k) {
        RecordedCall c;
        c.k = k;
        memcpy(&c.rec, host + ks.natives[k].record_offset, sizeof c.rec);
        if (!c.rec.executed) continue;
        if (c.rec.index < 0 || c.rec.index >= ks.native_sites) return fail("internal: native call record names no call site");
        c.func = &ks.natives[c.rec.index].func;
        calls->push_back(c);
    }
    std::sort(calls->begin(), calls->end(), [](const RecordedCall &x, const RecordedCall &y) { return x.rec.pad < y.rec.pad; });
    return 0;
}

// Is the call `c' recorded by a closure's render kernel the call `m' the main code has already made this frame?  The render
// kernel evaluates the main filter's code once more (it computes the closure's arguments), native calls included: those are
// the same calls on the same images -- in the reference the closure's argument simply *is* the image the main code computed,
// and its cache would answer (native-filters/cache.c:110-147).  Scalars by their bits, images by what they refer to: an input
// image or closure by its handle, a native result by the main call its own producer was matched with (`alias': render
// kernel's entry -> main's image-table slot, -1 unmatched).
static bool same_native_call(const RecordedCall &c, const RecordedCall &m, const std::vector<int> &alias, int closure_slot_base) {
    if (*c.func != *m.func || c.rec.nargs != m.rec.nargs) return false;
    for (int i = 0; i < c.rec.nargs && i < 4; ++i) {
        const HNativeArg &x = c.rec.args[i], &y = m.rec.args[i];
        if (x.kind != y.kind) return false;
        if (x.kind != 2) {
            if (x.i != y.i || memcmp(&x.f, &y.f, sizeof x.f) != 0) return false;
            continue;
        }
        int idx = x.img.idx;
        const int rel = idx - closure_slot_base;
        if (rel >= 0 && rel < (int)alias.size()) {
            if (alias[rel] < 0) return false;
            idx = alias[rel];
        }
        if (idx != y.img.idx || x.img.pw != y.img.pw || x.img.ph != y.img.ph || x.img.resized != y.img.resized ||
            memcmp(&x.img.xf, &y.img.xf, sizeof x.img.xf) != 0 || memcmp(&x.img.yf, &y.img.yf, sizeof x.img.yf) != 0)
            return false;
    }
    return true;
}

// `main_done': the main code's calls run so far this frame (their maps are valid)
static int render_closure(mmhip_invocation *inv, mmhip_filter *f, int cid, const HArgs &main_args, hipStream_t s,
                          const std::vector<RecordedCall> &main_done) {
    mmhip_closure_kernel &ck = f->closures[cid];
    auto &st = inv->closure_state[cid];
    const int w = main_args.render_width, h = main_args.render_height;
    if (st.map && (st.w != w || st.h != h)) {      // the map and the closure's own native maps follow the render size
        HIP_TRY(hipDeviceSynchronize());
        st.map.reset();
        for (DeviceBuffer &m : st.native_results) m.reset();
    }
    if (!st.map) {
        HIP_TRY(st.map.grow((size_t)w * h * 16));
        st.w = w;
        st.h = h;
    }
    if (grow_launch_buffers(st.launch, ck.ks, w, h, false, s) != 0) return -1;
    // (t and frame stay the frame's own: the closure's *arguments* are values of the main filter's code at the current
    // time; the closure's body is lowered with t = 0.0 and frame = 0 as literals, lower.cpp native_image_argument)
    HArgs a = main_args;
    a.region_x = a.region_y = 0;
    a.region_width = w;
    a.region_height = h;
    a.sampling_offset_x = a.sampling_offset_y = 0.0f;
    a.first_row = 0;
    a.num_rows = h;
    a.output_bpp = 4;
    a.row_stride = w * 4;
    a.floatmap = 1;
    a.out = st.map.get();
    a.xtab = st.launch.xtab.get<float>();
    a.ytab = st.launch.ytab.get<float>();
    const LaunchGeometry geo = launch_geometry(ck.ks, w, h);
    a.ppt = geo.ppt;
    a.tiles_magic = geo.tiles_magic;
    char *xy = st.launch.xy.get<char>();
    void *params[] = {&a, &xy};
    const int n = std::max(w, h);
    a.native_slot_base = st.native_slot_base;
    HIP_TRY(hipModuleLaunchKernel(ck.f_pro, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, s, params, nullptr));
    if (!ck.ks.natives.empty()) {
        // The closure's own calc_lines starts with its init_frame, and that is where *its* native filters run
        // (builtins.c:273-298 -> new_template.c.in:314-337): the records its prologue just wrote, each executed call into a
        // map of the closure's own.  Like the closure image itself these are recomputed on every render (the reference
        // gives the closure a fresh id: nothing of it is ever found in the cache).
        std::vector<char> host(ck.ks.xy_bytes);
        HIP_TRY(hipMemcpyAsync(host.data(), xy, host.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<RecordedCall> calls;
        if (recorded_calls(ck.ks, host.data(), &calls) != 0) return -1;
        std::vector<int> alias(ck.ks.natives.size(), -1);
        for (const RecordedCall &call : calls) {
            const size_t k = call.k;
            const HNativeRec &rec = call.rec;
            // a call of the main code's copy: the main code has its result already (same_native_call)
            bool aliased = false;
            for (const RecordedCall &m : main_done) {
                const int mslot = inv->native_slot_base + (int)m.k;
                const NativeEntry &me = inv->natives[m.k];
                if (!same_native_call(call, m, alias, st.native_slot_base) || !me.map || inv->images[mslot].kind != IMG_FLOATMAP ||
                    inv->images[mslot].w != w || inv->images[mslot].h != h || me.rows.first > 0 || me.rows.second < h)
                    continue;
                inv->images[st.native_slot_base + (int)k] = inv->images[mslot];      // the same map under the render kernel's handle
                alias[k] = mslot;
                aliased = true;
                break;
            }
            if (aliased) continue;
            for (int i = 0; i < rec.nargs && i < 4; ++i)
                if (rec.args[i].kind == 2 && rec.args[i].img.idx <= -2)
                    return fail("a filter closure rendered for a native filter hands another closure to a native filter: not supported");
            HIP_TRY(st.native_results[k].grow((size_t)w * h * 16));
            std::string err;
            int lo = 0, hi = h;
            if (run_native_filter(*call.func, rec, inv->images, w, h, st.native_results[k].get<float>(), inv->ws, s, &err, &lo, &hi) != 0)
                return fail(err);
            inv->images[st.native_slot_base + (int)k] = floatmap_desc(st.native_results[k].get(), w, h);
        }
        if (upload_image_table(inv, s) != 0) return -1;
    }
    HIP_TRY(hipModuleLaunchKernel(ck.f_pix, (unsigned)geo.nwg, 1, 1, 256, 1, 1, 0, s, params, nullptr));
    return 0;
}

// Direct output (hipgen.cpp find_direct_native): the pixel is native result k sampled at (x, y).
// If every sample position of this launch is the pixel's own centre -- get_floatmap_pixel's
// lrintf(ax x + bx) (builtins.c:247-265) evaluated here for each column and row with the
// coordinates the prologue just computed -- the native filter may write the RGBA8 pixels itself.
// Waits for `s', and with it for what the caller queued there before (the frame constants' read-back).
bool direct_output_wanted(const mmhip_filter *f, const HArgs &a) {
    return f->ks.direct_native >= 0 && !a.floatmap && a.output_bpp == 4 && (a.row_stride & 3) == 0 && ((uintptr_t)a.out & 3) == 0 &&
           !getenv("MMHIP_NO_DIRECT_NATIVE");
}

// xt, yt: the launch's coordinate tables as the prologue wrote them
bool samples_own_pixels(const HArgs &a, const std::vector<float> &xt, const std::vector<float> &yt) {
    const HImageDesc m = floatmap_desc(nullptr, a.render_width, a.render_height);
    for (int c = 0; c < a.region_width; ++c)
        if (lrintf(m.ax * xt[c] + m.bx) != (long)a.region_x + c) return false;
    for (int r = 0; r < a.num_rows; ++r)
        if (lrintf(m.ay * yt[r] + m.by) != (long)a.first_row + r) return false;
    return true;
}

// queues the copies; the tables are there once `s' has been waited for
int read_coordinate_tables(const HArgs &a, hipStream_t s, std::vector<float> *xt, std::vector<float> *yt) {
    xt->resize(a.region_width);
    yt->resize(a.num_rows);
    HIP_TRY(hipMemcpyAsync(xt->data(), a.xtab, xt->size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(yt->data(), a.ytab, yt->size() * sizeof(float), hipMemcpyDeviceToHost, s));
    return 0;
}

static int direct_output(const mmhip_filter *f, const HArgs &a, hipStream_t s, NativeDirectOut *direct) {
    const bool try_direct = direct_output_wanted(f, a);
    std::vector<float> xt, yt;
    if (try_direct && read_coordinate_tables(a, s, &xt, &yt) != 0) return -1;
    HIP_TRY(hipStreamSynchronize(s));
    if (!try_direct) return 0;
    if (!samples_own_pixels(a, xt, yt)) return 0;
    direct->out = a.out;
    direct->row_stride = a.row_stride;
    direct->first_row = a.first_row;
    direct->num_rows = a.num_rows;
    direct->region_x = a.region_x;
    direct->region_w = a.region_width;
    return 0;
}

// Closure images among the arguments (index -2 - id, mm_closure_image): rendered into float maps now and
// handed to the native filter as such, in `images_k' (a copy of the image table, left empty when the call has
// none).  The reference gives every closure image a fresh id (image_new_id), so a call on a closure never hits
// the cache: always recomputed here too.
static int render_closure_args(mmhip_invocation *inv, mmhip_filter *f, const HArgs &a, hipStream_t s,
                               const std::vector<RecordedCall> &done, HNativeRec &rec, std::vector<HImageDesc> &images_k) {
    for (int i = 0; i < rec.nargs && i < 4; ++i) {
        HImage &img = rec.args[i].img;
        if (rec.args[i].kind != 2 || img.idx > -2) continue;
        const int cid = -2 - img.idx;
        if (cid >= (int)f->closures.size()) return fail("internal: closure image without a render kernel");
        if (render_closure(inv, f, cid, a, s, done) != 0) return -1;
        if (images_k.empty()) images_k = inv->images;
        img.idx = (int)images_k.size();
        img.pw = a.render_width;
        img.ph = a.render_height;
        img.xf = img.yf = 1.0f;      // a plain map: the closure's render kernel has applied the
        img.resized = 0;             // wrapper's factors to its coordinates already (lower.cpp)
        images_k.push_back(floatmap_desc(inv->closure_state[cid].map.get(), a.render_width, a.render_height));
    }
    return 0;
}

// MMHIP_NATIVE_FRAME_CURRENT: an argument that is a bound sequence (a drawable of more than one frame) is read at the
// render's frame number -- the call sees a one-frame view of it, in `images_k' (a copy of the image table, made here if
// the call has none yet).  `frame_key' becomes that frame number: part of what the memo and the direct output's `seen'
// record compare, so that one frame's result never answers for another's.  A frame the sequence does not have is an error.
int view_sequence_args(const mmhip_invocation *inv, int frame, const std::string &func, const HNativeRec &rec,
                              std::vector<HImageDesc> &images_k, int *frame_key) {
    *frame_key = NO_FRAME_KEY;
    if (inv->native_input_frame != MMHIP_NATIVE_FRAME_CURRENT) return 0;
    for (int i = 0; i < rec.nargs && i < 4; ++i) {
        const int idx = rec.args[i].img.idx;
        if (rec.args[i].kind != 2 || idx < 0 || idx >= inv->native_slot_base) continue;
        const HImageDesc &d = inv->images[idx];
        if (d.kind != IMG_DRAWABLE || d.num_frames <= 1) continue;
        if (frame < 0 || frame >= d.num_frames)
            return fail((func == "RENDER" ? std::string("render()") : func.rfind("native_filter_", 0) == 0 ? func.substr(14) : func) + ": frame " + std::to_string(frame) + " is outside the input sequence (" + std::to_string(d.num_frames) +
                        " frames; native input frame mode `current')");
        if (images_k.empty()) images_k = inv->images;
        HImageDesc &v = images_k[idx];
        v.data = (const char *)d.data + (size_t)frame * d.w * d.h * 4;
        v.num_frames = 1;
        *frame_key = frame;
    }
    return 0;
}

// memo (native-filters/cache.c:110-147): same arguments on unchanged inputs -> keep the map.  `deps' receives the
// generations of the native maps among the call's image arguments (cache.c keys on image ids).
static bool memo_hit(const mmhip_invocation *inv, const NativeEntry &e, const HNativeRec &rec, int frame_key, int want_lo, int want_hi,
                     std::vector<unsigned long long> *deps) {
    for (int i = 0; i < rec.nargs && i < 4; ++i)
        if (rec.args[i].kind == 2 && rec.args[i].img.idx >= inv->native_slot_base &&
            rec.args[i].img.idx < inv->native_slot_base + (int)inv->natives.size())
            deps->push_back(inv->natives[rec.args[i].img.idx - inv->native_slot_base].gen);
    return e.map && e.memo_gen == inv->input_generation && e.memo_frame == frame_key && memcmp(&e.memo, &rec, sizeof rec) == 0 && e.memo_deps == *deps &&
           e.rows.first <= want_lo && e.rows.second >= want_hi;
}

// Native entry k's map goes (the caller has waited for what reads it), and with it its memo and its image-table entry.
static void drop_native_map(mmhip_invocation *inv, size_t k, bool *table_changed) {
    NativeEntry &e = inv->natives[k];
    e.map.reset();
    e.memo_gen = e.seen_gen = ~0ULL;
    e.rows = {0, 0};
    HImageDesc &d = inv->images[inv->native_slot_base + (int)k];
    d.kind = IMG_NULL;
    d.data = nullptr;
    *table_changed = true;
}

// what the native filters of `f' run with (render_closure runs its native filters with these too)
void set_native_env(mmhip_invocation *inv, const mmhip_filter *f, bool gauss_tolerance) {
    inv->ws.env.supersampling = f->kopt.supersampling;
    inv->ws.env.edge_x = f->kopt.edge_x;
    inv->ws.env.edge_y = f->kopt.edge_y;
    inv->ws.env.edge_color_x = inv->edge_color_x;
    inv->ws.env.edge_color_y = inv->edge_color_y;
    inv->ws.gauss_tolerance = gauss_tolerance;
}

static int run_natives(mmhip_invocation *inv, mmhip_filter *f, const HArgs &a, hipStream_t s, bool *direct_written) {
    std::vector<char> host(f->ks.xy_bytes);
    HIP_TRY(hipMemcpyAsync(host.data(), inv->launch.xy.get(), host.size(), hipMemcpyDeviceToHost, s));
    NativeDirectOut direct;
    if (direct_output(f, a, s, &direct) != 0) return -1;
    set_native_env(inv, f, f->opts.gauss_mode == MMHIP_GAUSS_TOLERANCE);
    // rows of the maps this launch may read: everything, or -- opt-in, full-frame regions only --
    // the stripe being rendered (the filter samples the map within its own rows +- margin)
    int want_lo = 0, want_hi = a.render_height;
    if (inv->native_row_margin >= 0 && a.region_x == 0 && a.region_y == 0 && a.region_width == a.render_width &&
        a.region_height == a.render_height) {
        want_lo = std::max(0, a.first_row - inv->native_row_margin);
        want_hi = std::min(a.render_height, a.first_row + a.num_rows + inv->native_row_margin);
    }
    // A launch that covers the whole frame needs the map for nothing but the memo.  The first time
    // an argument set is seen it is therefore not written (16 of the second pass's 20 B/px); a
    // second request for the same set -- an animation that keeps the blur's arguments -- computes
    // it once more, with the map, and is memoised from then on.
    const bool whole = a.region_x == 0 && a.region_y == 0 && a.region_width == a.render_width &&
                       a.region_height == a.render_height && a.first_row == 0 && a.num_rows == a.render_height;
    bool table_changed = false;
    std::vector<RecordedCall> calls, done;      // done: calls whose maps stand (what a closure's render kernel may refer to)
    if (recorded_calls(f->ks, host.data(), &calls) != 0) return -1;
    for (const RecordedCall &call : calls) {
        const size_t k = call.k;
        NativeEntry &e = inv->natives[k];
        HNativeRec rec = call.rec;
        // A map belongs to the render size it was allocated for: the GIMP flow renders a small preview
        // and then the full image on one invocation (mathmap.c:2191-2223).  On a change the map is
        // reallocated and everything remembered about it dropped.
        if (e.map && (e.w != a.render_width || e.h != a.render_height)) {
            HIP_TRY(hipDeviceSynchronize());
            drop_native_map(inv, k, &table_changed);
        }
        std::vector<HImageDesc> images_k;
        if (render_closure_args(inv, f, a, s, done, rec, images_k) != 0) return -1;
        const bool closure_args = !images_k.empty();      // never memoised (render_closure_args)
        int frame_key = NO_FRAME_KEY;
        if (view_sequence_args(inv, a.frame, *call.func, rec, images_k, &frame_key) != 0) return -1;
        std::vector<unsigned long long> deps;
        if (memo_hit(inv, e, rec, frame_key, want_lo, want_hi, &deps) && !closure_args) {
            ++inv->native_memo_hits;
            done.push_back(call);
            continue;
        }
        HIP_TRY(e.map.grow((size_t)a.render_width * a.render_height * 16));
        e.w = a.render_width;
        e.h = a.render_height;
        std::string err;
        int got_lo = want_lo, got_hi = want_hi;
        NativeDirectOut *dk = (direct.out && (int)k == f->ks.direct_native) ? &direct : nullptr;
        if (dk) {
            dk->skip_map = whole && !(e.seen_gen == inv->input_generation && e.seen_frame == frame_key && e.memo_deps == deps &&
                                      memcmp(&e.seen, &rec, sizeof rec) == 0);
            e.seen = rec;
            e.seen_frame = frame_key;
            e.seen_gen = inv->input_generation;
        }
        if (run_native_filter(*call.func, rec, images_k.empty() ? inv->images : images_k, a.render_width, a.render_height,
                              e.map.get<float>(), inv->ws, s, &err, &got_lo, &got_hi, dk) != 0)
            return fail(err);
        e.gen = ++inv->native_gen_counter;
        e.memo_deps = deps;
        if (dk && dk->written) *direct_written = true;
        if (dk && dk->written && dk->tolerance) ++inv->tolerance_blur_launches;
        if (dk && dk->written && dk->skip_map) {       // nothing to memoise, no map to describe
            e.memo_gen = ~0ULL;
            e.rows = {0, 0};
            continue;
        }
        inv->images[inv->native_slot_base + (int)k] = floatmap_desc(e.map.get(), a.render_width, a.render_height);
        e.memo = rec;
        e.memo_frame = frame_key;
        e.memo_gen = inv->input_generation;
        e.rows = {got_lo, got_hi};
        table_changed = true;
        done.push_back(call);
    }
    // dynamic entries this frame did not use (the loop ran fewer times than before): their maps go back (a map is
    // 16 B per pixel of the frame; sixteen of them at 16384^2 are 69 GB)
    if (f->ks.native_sites < (int)f->ks.natives.size()) {
        std::vector<char> used(f->ks.natives.size(), 0);
        for (const RecordedCall &call : calls) used[call.k] = 1;
        for (size_t k = (size_t)f->ks.native_sites; k < f->ks.natives.size(); ++k) {
            if (used[k] || !inv->natives[k].map) continue;
            HIP_TRY(hipStreamSynchronize(s));
            drop_native_map(inv, k, &table_changed);
        }
    }
    if (table_changed && upload_image_table(inv, s) != 0) return -1;
    return 0;
}

// Specialisation of a filter that has no source text (IR imported through the reference-ABI tier or
// mmhip_compile_ir_json): reload its own IR dump, replace the scalar USERVAL_*_ACCESS reads by the
// literals, and run the same constant propagation / folding as the source-level variant.
static void bake_uservals(Block &b, const std::map<int, Primary> &consts) {
    for (Stmt *st : b) {
        if (st->kind == Stmt::Assign && st->rhs.kind == Rhs::Op && st->rhs.args.size() == 1 &&
            st->rhs.args[0].kind == Primary::IntConst) {
            const char *n = st->rhs.op->cname;
            if (!strcmp(n, "USERVAL_INT_ACCESS") || !strcmp(n, "USERVAL_FLOAT_ACCESS") || !strcmp(n, "USERVAL_BOOL_ACCESS")) {
                auto it = consts.find(st->rhs.args[0].i);
                if (it != consts.end()) {
                    st->rhs = Rhs::P(it->second);
                    st->rhs.prim.of_variable = true;
                }
            }
        }
        if (st->kind == Stmt::If) { bake_uservals(st->then_, consts); bake_uservals(st->else_, consts); }
        if (st->kind == Stmt::While) bake_uservals(st->body, consts);
    }
}

static mmhip_filter *compile_ir_specialized(const mmhip_filter *f, const std::map<int, Primary> &consts, bool peel = true) {
    mmhip_filter *sp = mmhip_filter_new_empty();
    try {
        sp->code.reset(new FilterCode());
        load_ir_json(sp->module, *sp->code, (f->ir_json_raw.empty() ? f->ir_json : f->ir_json_raw).c_str());
        bake_uservals(sp->code->body, consts);
        specialize_constants(*sp->code);
        const bool peeled = peel && pair_peel_enabled() && peel_first_trips(*sp->code);      // a trial, as in compile_source
        for (auto &sub : sp->code->closure_renders) {
            bake_uservals(sub->body, consts);
            specialize_constants(*sub);
        }
        std::string err;
        if (!mmhip_filter_finalize(sp, f->kopt, &err)) throw CompileError(err);
        if (peeled && !sp->ks.pair_exit) {
            mmhip_filter_free(sp);
            return compile_ir_specialized(f, consts, false);
        }
        sp->opts = f->opts;
        sp->opts.specialize_uservals = 0;
    } catch (const std::exception &e) {
        g_err = e.what();
        mmhip_filter_free(sp);
        return nullptr;
    }
    return sp;
}

// The variant of a compiled filter with n scalar user values (index, value) baked in as literals: what
// active_filter() builds lazily for a value set, for filters of either origin (source text or IR dump).
static mmhip_filter *compile_variant(const mmhip_filter *f, const std::map<int, Primary> &consts) {
    mmhip_options o = f->opts;
    o.specialize_uservals = 0;
    return f->source.empty() ? compile_ir_specialized(f, consts) : compile_source(f->source.c_str(), &o, &consts);
}

mmhip_filter *mmhip_filter_specialized(const mmhip_filter *f, int n, const int *indices, const double *values) {
    std::map<int, Primary> consts;
    if (!scalar_constants(f->module.main->uservals, n, indices, values, &consts)) return nullptr;
    return compile_variant(f, consts);
}

// The kernel set to launch: the generic filter, or -- with options.specialize_uservals -- a
// variant with the current scalar user values baked in as literals (built on first use per
// value set, cached on the filter and on disk through the hiprtc cache).
mmhip_filter *active_filter(mmhip_invocation *inv, int frame, float t) {
    mmhip_filter *f = inv->f;
    if (!f->specialize || !f->ks.natives.empty() || (f->source.empty() && f->ir_json.empty() && f->ir_json_raw.empty())) return f;
    g_err.clear();
    const auto &uvs = f->module.main->uservals;
    std::string key;
    std::map<int, Primary> consts;
    for (const UservalInfo &u : uvs) {
        if (u.kind == UvKind::Int || u.kind == UvKind::Bool) consts[u.index] = Primary::I(inv->uv[u.index].i);
        else if (u.kind == UvKind::Float) consts[u.index] = Primary::F(inv->uv[u.index].f);
        else continue;
        key.append((const char *)&inv->uv[u.index], sizeof(HUserval));
    }
    if (consts.empty()) return f;
    auto it = f->spec_cache.find(key);
    if (it != f->spec_cache.end()) return it->second ? it->second : f;
    // a host that changes values on every render (interactive sliders) should not pay a JIT each
    // time: build the variant on the spec_min_uses-th render with the same values
    // A "use" is a render of a new frame with these values: the bands of one frame count once, so a
    // host that animates a user value (new values every frame, several calc_lines bands each) never
    // triggers a JIT per frame; an animation over t with fixed values specialises at its 2nd frame.
    if (f->spec_min_uses > 1) {
        if (f->spec_uses.size() > 1024) f->spec_uses.clear();
        auto &u = f->spec_uses[key];
        if (u.count == 0 || u.frame != frame || u.t != t) {
            ++u.count;
            u.frame = frame;
            u.t = t;
        }
        if (u.count < f->spec_min_uses) return f;
    }
    f->spec_uses.erase(key);
    mmhip_filter *sp = compile_variant(f, consts);
    if (sp && mmhip_filter_jit(sp, 1) < 0) { mmhip_filter_free(sp); sp = nullptr; }
    f->spec_cache[key] = sp;          // nullptr = fall back to the generic kernel for this value set
    return sp ? sp : f;
}

// mm_args of a render of rows [first_row, last_row) of a region, without the launch's own buffers and geometry
HArgs render_args(const mmhip_invocation *inv, int frame, float t, int region_x, int region_y, int region_w, int region_h,
                         int first_row, int last_row, void *out_device, int row_stride, int bpp, int floatmap) {
    HArgs a{};
    a.img_width = inv->img_w;
    a.img_height = inv->img_h;
    a.render_width = inv->render_w;
    a.render_height = inv->render_h;
    a.frame_render_width = inv->render_w;     // invocation_new_frame, mathmap_common.c:805-806
    a.frame_render_height = inv->render_h;
    a.t = t;
    a.frame = frame;
    a.R = (float)sqrt(2.0);                   // mathmap_common.c:770
    a.region_x = region_x;
    a.region_y = region_y;
    a.region_width = region_w;
    a.region_height = region_h;
    a.sampling_offset_x = inv->sampling_offset_x;
    a.sampling_offset_y = inv->sampling_offset_y;
    a.first_row = first_row;
    a.num_rows = last_row - first_row;
    a.output_bpp = bpp;
    a.row_stride = row_stride;
    a.floatmap = floatmap;
    a.edge_color_x = inv->edge_color_x;
    a.edge_color_y = inv->edge_color_y;
    a.uservals = inv->d_uv.get<HUserval>();
    a.images = inv->d_images.get<HImageDesc>();
    a.num_images = (uint32_t)inv->images.size();
    a.curves = inv->d_curves.get();
    a.gradients = inv->d_gradients.get();
    a.out = out_device;
    a.native_slot_base = inv->native_slot_base;
    return a;
}

// new_template.c.in:238-239: the rows of a call, clamped to the region; false where none are left
bool clamp_rows(int region_y, int region_h, int *first_row, int *last_row) {
    if (*first_row < 0) *first_row = 0;
    if (*last_row > region_y + region_h) *last_row = region_y + region_h;
    return *last_row > *first_row;
}

int mmhip_render(mmhip_invocation *inv, int frame, float t, int region_x, int region_y, int region_w, int region_h,
                 int first_row, int last_row, void *out_device, int row_stride, int bpp, int floatmap, void *stream) {
    mmhip_filter *f = active_filter(inv, frame, t);
    hipStream_t s = stream ? (hipStream_t)stream : inv->stream;
    if (bpp < 1 || bpp > 4) return fail("output_bpp must be 1..4");
    if (region_w <= 0 || region_h <= 0) return fail("empty region");
    if (!clamp_rows(region_y, region_h, &first_row, &last_row)) return 0;
    if (upload_tables(inv, s) != 0) return -1;

    HArgs a = render_args(inv, frame, t, region_x, region_y, region_w, region_h, first_row, last_row, out_device, row_stride, bpp, floatmap);
    const size_t rowtab_bytes = inv->launch.rowtab.bytes;
    if (grow_launch_buffers(inv->launch, f->ks, region_w, a.num_rows, f->ks.row_values > 0, s) != 0) return -1;
    if (inv->launch.rowtab.bytes != rowtab_bytes) inv->pro_filter = nullptr;     // the per-row table is new: fill it
    a.xtab = inv->launch.xtab.get<float>();
    a.ytab = inv->launch.ytab.get<float>();
    if (f->ks.row_values > 0) a.rowtab = inv->launch.rowtab.get<float>();
    char *xy = inv->launch.xy.get<char>();
    void *params[] = {&a, &xy};
    bool direct_written = false;      // a native filter wrote this launch's pixels itself (run_natives)
    {
        // The prologue's outputs (frame constants, coordinate tables) depend on the filter, the
        // geometry, the user values / image table and -- only if its code reads them -- t and
        // frame: while none of those changed since it last ran on these buffers, skip the launch
        // (an animation of a filter whose constants do not involve t pays for it once).
        HArgs key = a;
        key.out = nullptr;
        key.row_stride = key.output_bpp = key.floatmap = key.ppt = 0;
        key.tiles_magic = 0;
        if (!f->ks.prologue_uses_time) { key.t = 0.0f; key.frame = 0; }
        const bool fresh = f->ks.natives.empty() && inv->pro_filter == f && inv->pro_stream == (void *)s &&
                           inv->pro_generation == inv->table_generation &&
                           memcmp(&key, &inv->pro_args, sizeof key) == 0;
        if (!fresh) {
            int n = std::max(region_w, a.num_rows);
            HIP_TRY(hipModuleLaunchKernel(f->f_pro, (unsigned)((n + 255) / 256), 1, 1, 256, 1, 1, 0, s, params, nullptr));
            ++inv->prologue_launches;
            // the per-row slice (x-const code): once per row of the launch, after the frame constants it reads
            if (f->ks.row_values > 0)
                HIP_TRY(hipModuleLaunchKernel(f->f_rows, (unsigned)((a.num_rows + 255) / 256), 1, 1, 256, 1, 1, 0, s, params, nullptr));
            if (!f->ks.natives.empty() && run_natives(inv, f, a, s, &direct_written) != 0) return -1;
            inv->pro_args = key;
            inv->pro_filter = f;
            inv->pro_stream = (void *)s;
            inv->pro_generation = inv->table_generation;
        }
    }
    const LaunchGeometry geo = launch_geometry(f->ks, region_w, a.num_rows);
    const long nwg = geo.nwg;
    if (nwg > 0x7fffffffL) return fail("region too large for one launch");
    a.ppt = geo.ppt;
    a.tiles_magic = geo.tiles_magic;
    if (direct_written) ++inv->direct_native_launches;
    return timed_pixel_launch(inv, direct_written ? nullptr : f->f_pix, (unsigned)nwg, 1, params, s);
}

// call_invocation with supersampling (mathmap_common.c:880-927), whole region on the GPU.
// The filter must have been compiled with options.supersampling = 1 (nearest fetch without
// the +0.5, builtins.c:154-158).
int mmhip_render_supersampled(mmhip_invocation *inv, int frame, float t, int region_x, int region_y, int region_w,
                              int region_h, void *out_device, int row_stride, int bpp, void *stream) {
    hipStream_t s = stream ? (hipStream_t)stream : inv->stream;
    const size_t long_bytes = (size_t)(region_w + 1) * bpp * region_h;
    const size_t short_bytes = (size_t)region_w * bpp * region_h;
    // own allocation: the nested renders run native filters, which reallocate inv->ws
    if (inv->ss_lines.grow(long_bytes + short_bytes, hipDeviceSynchronize) != hipSuccess)
        return fail("out of device memory for the supersampling lines");
    unsigned char *tmp = inv->ss_lines.get<unsigned char>();
    SamplingOffsetGuard offsets(inv);
    // long slice: region_width + 1 columns, offsets -0.5 (invocation_init_slice, :892)
    offsets.set(-0.5f);
    int rc = mmhip_render(inv, frame, t, region_x, region_y, region_w + 1, region_h, region_y, region_y + region_h, tmp,
                          (region_w + 1) * bpp, bpp, 0, s);
    offsets.set(0.f);
    if (rc == 0)
        rc = mmhip_render(inv, frame, t, region_x, region_y, region_w, region_h, region_y, region_y + region_h,
                          tmp + long_bytes, region_w * bpp, bpp, 0, s);
    if (rc != 0) return rc;
    launch_supersample_combine(tmp, tmp + long_bytes, (unsigned char *)out_device, region_w, region_h, bpp, row_stride, s);
    return 0;
}

int mmhip_sync(mmhip_invocation *inv) {
    HIP_TRY(hipStreamSynchronize(inv->stream));
    return 0;
}

int mmhip_render_host(mmhip_invocation *inv, int frame, float t, uint8_t *out_rgba) {
    size_t bytes = (size_t)inv->render_w * inv->render_h * 4;
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    int rc = mmhip_render(inv, frame, t, 0, 0, inv->render_w, inv->render_h, 0, inv->render_h, d, inv->render_w * 4, 4, 0,
                          nullptr);
    if (rc == 0) {
        hipError_t e = hipStreamSynchronize(inv->stream);
        if (e == hipSuccess) e = hipMemcpy(out_rgba, d, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(std::string("render: ") + hipGetErrorString(e));
    }
    (void)hipFree(d);
    return rc;
}

void *mmhip_device_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { fail("hipMalloc failed"); return nullptr; }
    return p;
}
void mmhip_device_free(void *p) { (void)hipFree(p); }
int mmhip_copy_to_host(void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}
int mmhip_copy_to_device(void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
int mmhip_set_device(int ordinal) {
    HIP_TRY(hipSetDevice(ordinal));
    return 0;
}
int mmhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
