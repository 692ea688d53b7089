// IR -> HIP C++ source.  See hipgen.h.
//
// Shape of the generated translation unit:
//
//   #define MM_INTERSAMPLE / MM_EDGE_X / MM_TILE_W / MM_UNROLL ...   (compile-time options)
//   <mm_fastmath.h + tables, mm_gslmath.h>                           (float-argument libm, GSL ops)
//   <mm_device.h>  [<mm_noise_device.h> + gradient table]            (device runtime)
//   extern "C" __global__ void mm_prologue(mm_args A, char *XY)      lane 0: frame-constant values ->
//                                                                    constant buffer, native-filter call
//                                                                    records; all lanes: x / y tables
//   extern "C" __global__ void mm_pixels(mm_args A, const char *XY)  pixel kernel, one of two shapes:
//       loop shape   : frame constants + image descriptors loaded once, then A.ppt rows per work-item,
//                      MM_UNROLL pixels evaluated back to back (stores deferred), with a branch-free
//                      "hot" copy of the loop when every fetch reads a bound drawable
//       single shape : one pixel per work-item, lazy scalar loads (large bodies: no SGPR spills)
//       pair mode    : loop shape for small arithmetic-only bodies -- two vertically adjacent pixels as
//                      pairs of values in lockstep (two interleaved instruction streams), hipgen_pair.cpp
//
// Two more modules are made of the same statements: the clip variant (mm_*_clip: this text with the kernels' heads
// replaced, clip_kernel_source) and, generated on demand under KernelOptions::shutter, the shutter variant -- the clip
// forms of the prologue and the per-row slice, and mm_pixels_shutter: the single shape's body in a loop over a pixel's
// sub-samples (emit_shutter_pixel_kernel).  KernelOptions::sampled gives the same with mm_pixels_sampled, whose loop also
// walks a grid of sampling offsets (emit_sampled_pixel_kernel); with KernelOptions::refine the same kernel takes its pixels
// from a list (mm_pixels_refine).
//
// The environment hooks for experiments that alter this text are the fields of struct Knobs (hipgen_internal.h).
//
// Statement printing follows the reference's backends/cc.c:192-397 (one C variable
// per SSA value, phi copies at the end of branches / loop bodies), so the arithmetic
// the GPU executes is statement-for-statement the arithmetic gcc compiled for the
// cc backend.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>

#include "front.h"
#include "hipgen_internal.h"

namespace mm {
namespace hipgen {

std::optional<int> env_int(const char *name) {
    const char *e = getenv(name);
    return e ? std::optional<int>(atoi(e)) : std::nullopt;
}

std::string vname(const Value *v) {
    char buf[64];
    snprintf(buf, sizeof buf, "v%d_%d", v->var->id, v->index);
    return buf;
}

std::string ctype(const CompVar *v) {
    switch (v->type) {
        case Ty::Int: return "int";
        case Ty::Float: return "float";
        case Ty::Complex: return "mm_complex";
        case Ty::Color: return "color_t";
        case Ty::Curve:
        case Ty::Gradient: return "int";
        case Ty::Image: return "mm_image";
        case Ty::Tuple: return "mm_tup<" + std::to_string(v->tuple_len > 0 ? v->tuple_len : 4) + ">";
        case Ty::TreeVector:       // a tree vector's length is static (ir.cpp propagate_types): `len' floats
            if (v->tuple_len <= 0) throw CompileError("HIP backend: tree vector of unknown length");
            return "mm_tup<" + std::to_string(v->tuple_len) + ">";
        default: throw CompileError(std::string("HIP backend: unsupported variable type ") + ty_name(v->type));
    }
}

int type_size(const CompVar *v) {
    switch (v->type) {
        case Ty::Complex: return 8;
        case Ty::Image: return 24;
        case Ty::Tuple: return 4 * (v->tuple_len > 0 ? v->tuple_len : 4);
        case Ty::TreeVector: return 4 * std::max(v->tuple_len, 1);
        default: return 4;
    }
}

std::string float_literal(float f) {
    if (std::isnan(f)) return "__builtin_nan(\"\")";
    if (std::isinf(f)) return f > 0 ? "(1.0/0.0)" : "(-1.0/0.0)";
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", (double)f);
    std::string s = buf;
    if (s.find_first_of(".en") == std::string::npos) s += ".0";
    return s;
}

// The device function for a libm operator.  `f32`: the one for float arguments and a float result, where there is one
// whose value is (float)fn((double)f), bit for bit: sqrtf is correctly rounded; sin, cos, exp, log, pow are table-driven
// evaluations verified against glibc for every float below 2^22 (mm_fastmath.h, tools/verify_fastmath.c); asinh and acosh
// are the platform's double function and the list of the arguments where its float differs from glibc's
// (mm_libm_exceptions.h; the other one-argument functions have no such argument: tools/libm_exceptions.py); hypot is
// glibc's own arithmetic for two floats (mm_fastmath.h).
const char *libm_name(const char *cname, bool f32) {
    static const struct { const char *cname, *any, *f32; } table[] = {
        {"sqrt", "mm_sqrt", "mm_sqrt_f32"}, {"hypot", "mm_hypot", "mmf_hypot_f32"}, {"sin", "mm_sin", "mmf_sin_f32"},
        {"cos", "mm_cos", "mmf_cos_f32"}, {"tan", "mm_tan"}, {"asin", "mm_asin"}, {"acos", "mm_acos"}, {"atan", "mm_atan"},
        {"atan2", "mm_atan2"}, {"pow", "mm_pow", "mmf_pow_f32"}, {"exp", "mm_exp", "mmf_exp_f32"}, {"log", "mm_log", "mmf_log_f32"},
        {"sinh", "mm_sinh"}, {"cosh", "mm_cosh"}, {"tanh", "mm_tanh"}, {"asinh", "mm_asinh", "mmf_asinh_f32"},
        {"acosh", "mm_acosh", "mmf_acosh_f32"}, {"atanh", "mm_atanh"}, {"fabs", "mm_fabs"}, {"floor", "mm_floor"},
        {"ceil", "mm_ceil"}, {"GAMMA", "mm_gamma"}, {"gsl_sf_beta", "mm_beta"}};
    for (auto &t : table)
        if (!strcmp(t.cname, cname)) return f32 && t.f32 ? t.f32 : t.any;
    return nullptr;
}

bool is_truth_op(const char *cname) {
    return !strcmp(cname, "LESS") || !strcmp(cname, "LEQ") || !strcmp(cname, "EQ") || !strcmp(cname, "NOT");
}

bool is_pow2_divisor(float c) {
    int ex = 0;
    return std::isfinite(c) && c != 0.0f && std::fabs(std::frexp(c, &ex)) == 0.5f && ex > -100 && ex < 100;
}

const Primary *sqrt_less_pow2(const Rhs &r, float *kk) {
    if (strcmp(r.op->cname, "LESS") || r.args[0].kind != Primary::Val || !r.args[1].is_const()) return nullptr;
    const Stmt *d = r.args[0].value->def;
    const double k = r.args[1].kind == Primary::IntConst ? (double)r.args[1].i : r.args[1].kind == Primary::FloatConst ? (double)r.args[1].f : -1.0;
    int ex = 0;
    if (!(k > 0 && std::frexp(k, &ex) == 0.5 && ex > -50 && ex < 50)) return nullptr;
    if (!d || d->kind != Stmt::Assign || d->rhs.kind != Rhs::Op || strcmp(d->rhs.op->cname, "sqrt") || d->lhs->var->type != Ty::Float ||
        d->rhs.args[0].type() != Ty::Float || d->rhs.args[0].kind != Primary::Val)
        return nullptr;
    *kk = (float)(k * k);
    return &d->rhs.args[0];
}

// Is the float value provably >= +0 (or NaN)?  Squares of one value, non-negative literals,
// and sums / copies of such.  Products and sums are f32 here (the C type of float (op) float
// is promoted to double by the op macros only for libm calls, not for + and *).
bool nonneg_or_nan(const Value *v, int depth) {
    if (!v || depth > 16 || v->var->type != Ty::Float) return false;
    const Stmt *d = v->def;
    if (!d || d->kind != Stmt::Assign) return false;
    const Rhs &r = d->rhs;
    auto prim_ok = [&](const Primary &p) {
        if (p.kind == Primary::FloatConst) return p.f >= 0.0f && !std::signbit(p.f);
        if (p.kind == Primary::IntConst) return p.i >= 0;
        if (p.kind == Primary::Val) return nonneg_or_nan(p.value, depth + 1);
        return false;
    };
    if (r.kind == Rhs::Prim) return prim_ok(r.prim);
    if (r.kind != Rhs::Op) return false;
    if (!strcmp(r.op->cname, "MUL") && r.args.size() == 2 && r.args[0].kind == Primary::Val && r.args[1].kind == Primary::Val &&
        r.args[0].value == r.args[1].value && r.args[0].value->var->type == Ty::Float)
        return true;
    if (!strcmp(r.op->cname, "ADD") && r.args.size() == 2) return prim_ok(r.args[0]) && prim_ok(r.args[1]);
    return false;
}

namespace {

// FNV-1a of a translation unit: its key, which is also the on-disk cache key of its code object
std::string text_key(const std::string &s) {
    unsigned long long h = 1469598103934665603ull;
    for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
    char buf[32];
    snprintf(buf, sizeof buf, "%016llx", h);
    return buf;
}

const std::string KERNEL = "extern \"C\" __global__ void __launch_bounds__(256) ";

// The device prelude of a kernel generated without KernelOptions::deep_inputs: mm_device.h less its MM_DEEP_INPUTS
// regions, each cut from its `#if MM_DEEP_INPUTS` line to its `#endif  // MM_DEEP_INPUTS` line.  That is the text the
// prelude had before the option existed, so such a kernel keeps its text, its key and its cached code object.
const std::string &plain_device_prelude() {
    static const std::string text = [] {
        const std::string open = "#if MM_DEEP_INPUTS\n", close = "#endif  // MM_DEEP_INPUTS\n";
        std::string s = device_prelude();
        for (size_t at; (at = s.find(open)) != std::string::npos;) {
            const size_t end = s.find(close, at);
            if (end == std::string::npos) throw CompileError("internal: mm_device.h: an MM_DEEP_INPUTS region without its #endif line");
            s.erase(at, end + close.size() - at);
        }
        return s;
    }();
    return text;
}

struct Generator {
    FilterCode &code;
    const KernelOptions &opt;
    const Knobs &knobs;
    std::ostringstream out;
    KernelSource ks;
    // filter_$name functions (FilterCode::functions): `fn_root` is the code whose functions are callable,
    // `in_function` is set while one of their bodies is printed
    FilterCode *fn_root = nullptr;
    bool in_function = false;
    // ---- which values live where (analyze_and_layout) ----
    std::vector<Value *> pro_defs, pix_defs, row_defs;
    std::set<Value *> pro_uses, pix_uses, row_uses;
    int pixel_stmts = 0, pixel_fetches = 0;    // size of the pixel slice (pixel_stats), once the row slice has left it
    std::map<Value *, int> transfer_off;       // hoisted values read by the pixel kernel
    std::map<const Stmt *, int> dual_base_off; // outermost loops of both slices with native calls: where the prologue leaves the
                                               // number of dynamic entries taken before the loop
    std::vector<Value *> transfer_order;
    std::map<const Stmt *, int> native_index;
    std::vector<Value *> row_transfer;         // row values the pixel slice uses, in table order
    // ---- fetches of the pixel kernel's loop shape ----
    std::set<const Value *> preloaded_desc;   // image values whose descriptor is loaded before the pixel loop
    std::set<const Stmt *> hot_sites;         // ORIG_VAL statements eligible for mm_orig_val_hot
    std::set<const Stmt *> hot_frame_sites;   // ... for mm_orig_val_hotf: the frame number differs per pixel
    std::map<const Stmt *, std::string> site_view;      // hot sites that read through a descriptor of their own
    bool hot_mode = false;
    // The hot fetch whose four channels are the filter's result, unchanged (the last statement of every pure
    // distortion: `in(f(xy))`): the hot loop then keeps the fetch's rounded byte sums and stores them directly
    // (mm_store_fetched_pixel) instead of dividing by 255, clamping and multiplying by 255 again.
    const Stmt *fetched_result = nullptr;
    // ---- sin / cos pairs of the scalar printer (join_sincos) ----
    struct SinCosRole { int id; bool first; };
    std::map<const Stmt *, SinCosRole> sincos_role;
    std::set<const Block *> sincos_scanned;
    int sincos_ids = 0;
    std::unique_ptr<PairMode> pair;           // pair mode, when the pixel loop is emitted in it (hipgen_pair.cpp)

    Generator(FilterCode &c, const KernelOptions &o, const Knobs &k) : code(c), opt(o), knobs(k) {}

    int function_index(const Filter *f) const {
        const FilterCode *root = fn_root ? fn_root : &code;
        for (size_t i = 0; i < root->functions.size(); ++i)
            if (root->functions[i]->filter == f) return (int)i;
        return -1;
    }

    std::string prim(const Primary &p, Slice) {
        switch (p.kind) {
            case Primary::Val: {
                const Value *v = p.value;
                if (v->index < 0) {
                    switch (v->var->type) {
                        case Ty::Image: return "UNINITED_IMAGE";
                        case Ty::Complex: return "mm_cmake(0.0f, 0.0f)";
                        case Ty::Tuple:
                        case Ty::TreeVector: return ctype(v->var) + "{}";
                        default: return "0";
                    }
                }
                if (pair && pair->is_uniform(v)) return "u" + vname(v);      // pair mode: wave-uniform loop value kept as a scalar
                return vname(v);
            }
            case Primary::IntConst: return p.i < 0 ? "(" + std::to_string(p.i) + ")" : std::to_string(p.i);
            case Primary::FloatConst: {
                std::string s = float_literal(p.f);
                return s[0] == '-' ? "(" + s + ")" : s;
            }
            case Primary::ComplexConst: return "COMPLEX(" + float_literal(p.f) + "," + float_literal(p.f2) + ")";
            case Primary::ColorConst: return std::to_string(p.color) + "u";
            default: return "0";
        }
    }

    // is `v` nameable from code of slice `sl` (defined there, or transferred into it)?
    bool value_visible(const Value *v, Slice sl) const {
        if (v->index < 0) return true;
        if (sl == PROLOGUE) return v->hoisted || v->loop_const;
        if (sl == ROWS) return v->row_const || transfer_off.count(const_cast<Value *>(v)) > 0;
        return !v->hoisted || transfer_off.count(const_cast<Value *>(v)) > 0;
    }

    // "mm_native_call(A, <record>, <counters>, k, " for a call site outside loops, the dynamic form for one inside
    std::string native_call_head(int k) const {
        const std::string ctr = "(int *)(XY + " + std::to_string(ks.native_ctr_offset) + "), ";
        if (!ks.natives[k].in_loop)
            return "mm_native_call(A, XY + " + std::to_string(ks.natives[k].record_offset) + ", " + ctr + std::to_string(k) + ", ";
        return "mm_native_call_in_loop(A, XY + " + std::to_string(ks.natives[ks.native_sites].record_offset) + ", " + ctr +
               std::to_string(k) + ", " + std::to_string(ks.native_sites) + ", ";
    }

    // A call of a native filter (or render()) by statement `stmt`: the prologue records it for the host; the pixel slice's
    // form of a call the prologue made from inside a loop of both slices (passes.cpp mark_dual_loops) is the handle of the
    // next dynamic entry; anywhere else the call cannot be made, because `why_not`.
    std::string native_call(const Rhs &r, Slice sl, const Stmt *stmt, const std::string &why_not) {
        auto it = native_index.find(stmt);
        if (it != native_index.end() && sl == PIXEL && stmt->hoisted && ks.natives[it->second].in_loop)
            return "mm_native_result_in_loop(A, mm_dyn_ctr, " + std::to_string(ks.native_sites) + ")";
        if (it == native_index.end() || sl != PROLOGUE) throw CompileError(why_not);
        std::string s = native_call_head(it->second) + std::to_string(r.args.size());
        for (size_t i = 0; i < r.args.size(); ++i) s += ", mm_narg(" + prim(r.args[i], sl) + ")";
        for (size_t i = r.args.size(); i < 4; ++i) s += ", mm_narg(0)";
        return s + ")";
    }

    std::string rhs(const Rhs &r, Slice sl, const Stmt *stmt, const CompVar *lhs) {
        switch (r.kind) {
            case Rhs::Prim: return prim(r.prim, sl);
            case Rhs::Internal: return r.internal;
            case Rhs::Tuple:
            case Rhs::TreeVector: {      // backends/cc.c:287-300: float tuple[n] = { args }; ALLOC_TREE_VECTOR(n, tuple)
                std::string s = "mm_tup<" + std::to_string(r.args.size()) + ">{{";
                for (size_t i = 0; i < r.args.size(); ++i) s += (i ? ", (float)(" : "(float)(") + prim(r.args[i], sl) + ")";
                return s + "}}";
            }
            case Rhs::Closure: {
                if (r.filter->kind == Filter::MathMap)      // index -2 - id: rendered for a native filter by the runtime
                    return "mm_closure_image(A, " + std::to_string(stmt ? stmt->closure_id : -1) + ")";
                return native_call(r, sl, stmt, "native filter `" + r.filter->name +
                                   "' is called with pixel-dependent arguments (or, with a filter closure among them, under pixel-dependent "
                                   "control); the HIP backend needs them frame-constant");
            }
            case Rhs::FilterCall: {
                // backends/cc.c:221-235: build the callee's argument block (output_make_mathmap_filter_closure), call
                // filter_$name(invocation, image, x, y, t, pools).  Here a statement expression around a template
                // instance: the template parameter is the call depth, so the call graph is a finite DAG (see emit_functions)
                const int k = function_index(r.filter);
                if (k < 0) throw CompileError("internal: call of filter `" + r.filter->name + "' without a function body");
                const size_t n = r.filter->uservals.size();
                if (r.args.size() != n + 3) throw CompileError("internal: malformed filter call");
                std::string e = "({ mm_uvarg mm_ca[" + std::to_string(n ? n : 1) + "]; ";
                for (size_t i = 0; i < n; ++i) {
                    const UservalInfo &u = r.filter->uservals[i];
                    const char *field = u.kind == UvKind::Float ? ".f = (float)(" : u.kind == UvKind::Color ? ".c = (color_t)(" : u.kind == UvKind::Image ? ".img = (" : ".i = (int)(";
                    e += "mm_ca[" + std::to_string(u.index) + "]" + field + prim(r.args[i], sl) + "); ";
                }
                e += "mm_filter_" + std::to_string(k) + "<" + (in_function ? "MM_D + 1" : "0") + ">(A, mm_ca, (float)(" + prim(r.args[n], sl) +
                     "), (float)(" + prim(r.args[n + 1], sl) + "), (float)(" + prim(r.args[n + 2], sl) + "), col, rl, mm_rand_ctr); })";
                return e;
            }
            case Rhs::Op: {
                const char *cn = r.op->cname;
                if (!strcmp(cn, "RENDER")) return native_call(r, sl, stmt, "render() needs frame-constant arguments in the HIP backend");
                // (the first two are unimplemented stubs in the reference too: opmacros.h:97-99)
                for (const char *bad : {"SOLVE_POLY_2", "SOLVE_POLY_3", "START_DEBUG_TUPLE", "SET_DEBUG_TUPLE_DATA", "OUTPUT_TUPLE"})
                    if (!strcmp(cn, bad)) throw CompileError(std::string("HIP backend: op ") + cn + " is not supported yet");
                if (!strcmp(cn, "PRINT_FLOAT") || !strcmp(cn, "NEWLINE")) return "0";
                // opmacros.h:189-190: the index is passed to a C `int' parameter (converted like FLOAT2INT), the value to a float
                if (!strcmp(cn, "TREE_VECTOR_NTH"))
                    return "mm_tv_nth(FLOAT2INT(" + prim(r.args[0], sl) + "), " + prim(r.args[1], sl) + ")";
                if (!strcmp(cn, "SET_TREE_VECTOR_NTH"))
                    return "mm_tv_set(FLOAT2INT(" + prim(r.args[0], sl) + "), " + prim(r.args[1], sl) + ", (float)(" + prim(r.args[2], sl) + "))";
                // escape-time test `sqrt(a) < 2^k`  ->  0 <= a < 4^k (exact, see mm_device.h)
                float kk = 0;
                const Primary *sq = opt.fast_math_exact ? sqrt_less_pow2(r, &kk) : nullptr;
                if (sq && value_visible(sq->value, sl)) {
                    // a sum of float squares is >= +0 or NaN, and `a < K*K` is false for NaN like
                    // sqrt(NaN) < K: the `a >= 0` half of the test is then dead
                    if (nonneg_or_nan(sq->value, 0)) return "((" + prim(*sq, sl) + ") < " + float_literal(kk) + "f)";
                    return "MM_SQRT_LESS_POW2(" + prim(*sq, sl) + ", " + float_literal(kk) + "f)";
                }
                if (sl == PIXEL && !strcmp(cn, "ORIG_VAL") && r.args.size() == 4) {      // the fetches of the loop shape
                    const std::string xyi = prim(r.args[0], sl) + ", " + prim(r.args[1], sl) + ", " + prim(r.args[2], sl) + ", ";
                    if (hot_mode && hot_frame_sites.count(stmt))      // frame number computed per pixel
                        return std::string(stmt == fetched_result ? "mm_tuple_of_sums(mm_rs[mm_u] = mm_orig_val_sums_hotf(A, " : "mm_orig_val_hotf(A, ") + xyi +
                               prim(r.args[3], sl) + ", " + vname(r.args[2].value) + "_desc, mm_bad)" + (stmt == fetched_result ? ")" : "");
                    if (hot_mode && stmt == fetched_result) return "mm_tuple_of_sums(mm_rs[mm_u] = mm_orig_val_sums_hot(A, " + xyi + site_desc(stmt) + ", mm_bad))";
                    if (hot_mode && hot_sites.count(stmt)) return "mm_orig_val_hot(A, " + xyi + site_desc(stmt) + ", mm_bad)";
                    if (r.args[2].kind == Primary::Val && preloaded_desc.count(r.args[2].value))
                        return "mm_orig_val_d(A, " + xyi + prim(r.args[3], sl) + ", " + vname(r.args[2].value) + "_desc)";
                }
                // x / c with c = +-2^k: x * (1/c) is the same correctly rounded value (scaling by a power of two
                // is exact or rounds identically, subnormals and overflow included), one multiply instead of
                // the ~10-instruction IEEE division sequence
                if (opt.fast_math_exact && !strcmp(cn, "DIV") && r.args.size() == 2 && r.args[1].kind == Primary::FloatConst &&
                    is_pow2_divisor(r.args[1].f))
                    return "((float)(" + prim(r.args[0], sl) + ") * " + float_literal(1.0f / r.args[1].f) + "f)";
                if (in_function && !strncmp(cn, "USERVAL_", 8) && r.args.size() == 1 && r.args[0].kind == Primary::IntConst) {
                    // inside filter_$name the user values are the call's arguments (new_template.c.in:375-422: the closure's args)
                    const char *field = !strcmp(cn, "USERVAL_FLOAT_ACCESS") ? "f" : !strcmp(cn, "USERVAL_COLOR_ACCESS") ? "c"
                                      : !strcmp(cn, "USERVAL_IMAGE_ACCESS") ? "img" : "i";
                    return "(UV[" + std::to_string(r.args[0].i) + "]." + field + ")";
                }
                std::string name = cn;
                bool floats = opt.fast_math_exact && !r.args.empty();      // float operands, and only where that is bit-identical
                for (const Primary &a : r.args) floats = floats && a.type() == Ty::Float;
                if (const char *lm = libm_name(cn, floats && lhs && lhs->type == Ty::Float)) name = lm;
                if (lhs && lhs->type == Ty::Int && (!strcmp(cn, "floor") || !strcmp(cn, "ceil")))
                    name = !strcmp(cn, "floor") ? "mm_floor_i" : "mm_ceil_i";      // x86 double -> int conversion
                if (floats && !strcmp(cn, "hypot") && !(lhs && lhs->type == Ty::Float)) name = "mm_hypot_ff";      // a double-typed result keeps the earlier form
                // a table read multiplies its argument before it truncates: a float where the argument is a variable's content
                const bool table_read = !strcmp(cn, "APPLY_CURVE") || !strcmp(cn, "APPLY_GRADIENT");
                std::string s = name + "(";
                for (size_t i = 0; i < r.args.size(); ++i)
                    s += (i ? "," : "") + std::string(table_read && r.args[i].kind == Primary::FloatConst && r.args[i].of_variable ? "(float)" : "") + prim(r.args[i], sl);
                return s + ")";
            }
            default: return "0";
        }
    }

    // ---- which values live where -------------------------------------------------------
    void collect_values(Block &b, Slice sl, std::vector<Value *> &defs, std::set<Value *> &uses) {
        auto use = [&](const Rhs &r) {
            if (r.kind == Rhs::Prim && r.prim.kind == Primary::Val) uses.insert(r.prim.value);
            for (const Primary &p : r.args)
                if (p.kind == Primary::Val) uses.insert(p.value);
        };
        for (Stmt *s : b) {
            bool mine = sl == PROLOGUE ? s->hoisted : sl == ROWS ? s->in_row : s->in_pixel;
            if (!mine) continue;
            switch (s->kind) {
                case Stmt::Assign: defs.push_back(s->lhs); use(s->rhs); break;
                case Stmt::Phi: defs.push_back(s->lhs); use(s->rhs); use(s->rhs2); break;
                case Stmt::If:
                    use(s->cond);
                    collect_values(s->then_, sl, defs, uses);
                    collect_values(s->else_, sl, defs, uses);
                    collect_values(s->phis, sl, defs, uses);
                    break;
                case Stmt::While:
                    collect_values(s->phis, sl, defs, uses);
                    use(s->cond);
                    collect_values(s->body, sl, defs, uses);
                    break;
                default: break;
            }
        }
    }

    // every statement of `b` and of the blocks inside it (not the phi lists), in program order; `f` says whether to go inside
    template <class F> static void each_stmt(const Block &b, F f) {
        for (const Stmt *s : b) {
            if (!f(s)) continue;
            if (s->kind == Stmt::If) { each_stmt(s->then_, f); each_stmt(s->else_, f); }
            if (s->kind == Stmt::While) each_stmt(s->body, f);
        }
    }
    static bool is_op(const Stmt *s, const char *cname, size_t n = 0) {      // an assignment of that operator (n > 0: of that prefix)
        return s->kind == Stmt::Assign && s->rhs.kind == Rhs::Op && (n ? !strncmp(s->rhs.op->cname, cname, n) : !strcmp(s->rhs.op->cname, cname));
    }
    static bool uses_noise(const Block &b) {
        bool noise = false;
        each_stmt(b, [&](const Stmt *s) { noise = noise || is_op(s, "libnoise_", 9); return true; });
        return noise;
    }

    std::string site_desc(const Stmt *s) const {
        auto it = site_view.find(s);
        return it != site_view.end() ? it->second : vname(s->rhs.args[2].value) + "_desc";
    }
    const Stmt *find_fetched_result() const {
        if (!opt.intersample || knobs.no_fetched_result) return nullptr;
        const Stmt *fetch = nullptr;
        for (int i = 0; i < 4; ++i) {
            const Value *v = code.result[i];
            const Stmt *d = v ? v->def : nullptr;
            // copies between the TUPLE_NTH and the result are gone after copy propagation
            if (!d || d->kind != Stmt::Assign || d->parent || !d->in_pixel || d->rhs.kind != Rhs::Op || strcmp(d->rhs.op->cname, "TUPLE_NTH") ||
                d->rhs.args[0].kind != Primary::Val || d->rhs.args[1].kind != Primary::IntConst || d->rhs.args[1].i != i)
                return nullptr;
            const Stmt *f = d->rhs.args[0].value->def;
            if (!f || f->parent || !(hot_sites.count(f) || hot_frame_sites.count(f)) || (fetch && f != fetch)) return nullptr;
            fetch = f;
        }
        return fetch;
    }

    // ORIG_VALs of the pixel slice whose image descriptor is preloaded: their "bound drawable" test can be made once
    // per work-item.  Two kinds of site.  The frame argument is a literal or a frame constant (hot_sites): "valid frame"
    // is tested there too, and the descriptor's hot pointer becomes that frame (mm_fetch_is_hot).  The sites of an image
    // that do not all name the same frame (a temporal blend) get a descriptor each (views).  The frame argument is
    // computed per pixel (hot_frame_sites, slit-scan): the fetch selects the frame itself, without a branch
    // (mm_orig_val_hotf); MMHIP_FRAME_HOT=0 leaves such a site to the generic fetch, as before there were sequences.
    // Appends one condition per site.
    void find_hot_fetches(const Block &b, std::vector<std::string> &views, std::vector<std::string> &conds) {
        std::vector<const Stmt *> sites;      // those ORIG_VALs, in program order
        each_stmt(b, [&](const Stmt *s) {
            if (s->in_pixel && is_op(s, "ORIG_VAL") && s->rhs.args.size() == 4 && s->rhs.args[2].kind == Primary::Val && preloaded_desc.count(s->rhs.args[2].value))
                sites.push_back(s);
            return s->in_pixel;
        });
        auto frame_const = [&](const Primary &f) { return f.is_const() || (f.kind == Primary::Val && transfer_off.count(f.value)); };
        std::map<const Value *, std::set<std::string>> frames_of;
        for (const Stmt *s : sites)
            if (frame_const(s->rhs.args[3])) frames_of[s->rhs.args[2].value].insert(prim(s->rhs.args[3], PIXEL));
        const bool frame_hot = knobs.frame_hot.value_or(1) != 0;
        for (const Stmt *s : sites) {
            const Primary &f = s->rhs.args[3];
            const std::string desc = vname(s->rhs.args[2].value) + "_desc";
            if (frame_const(f)) {
                hot_sites.insert(s);
                if (frames_of[s->rhs.args[2].value].size() > 1) {
                    const std::string view = "mm_fv" + std::to_string(site_view.size());
                    views.push_back("const mm_image_desc " + view + " = mm_frame_view(" + desc + ");");
                    site_view[s] = view;
                }
                conds.push_back("mm_fetch_is_hot(" + site_desc(s) + ", (int)(" + prim(f, PIXEL) + "))");
            } else if (frame_hot) {
                hot_frame_sites.insert(s);
                conds.push_back("mm_fetch_is_hot_any(" + desc + ")");
            }
        }
    }

    static bool hoisted_uses_time(const Block &b) {
        bool uses = false;
        each_stmt(b, [&](const Stmt *s) {
            uses = uses || (s->hoisted && s->kind == Stmt::Assign && s->rhs.kind == Rhs::Internal && (s->rhs.internal == "t" || s->rhs.internal == "frame"));
            return true;
        });
        return uses;
    }
    // pixel-slice statistics for the unroll choice
    static void pixel_stats(const Block &b, int &stmts, int &fetches) {
        each_stmt(b, [&](const Stmt *s) { stmts += s->in_pixel; fetches += s->in_pixel && is_op(s, "ORIG_VAL"); return s->in_pixel; });
    }

    // Filters that fetch pixels are bound by memory latency with one pixel in flight per
    // work-item (measured: a nearest fetch cost 0.25 ms at 8192^2 against 0.06 ms for the
    // store); evaluating several pixels back to back multiplies the loads in flight.  Measured at 8192^2
    // (tools/ab_unroll.sh, profiles/r02_ab_unroll.txt): Ident 0.233 / 0.204 / 0.205 ms and Pond 0.705 / 0.673 /
    // 0.752 ms for 2 / 4 / 8 pixels.  Large bodies are left alone: more code and registers cost more
    // occupancy than the overlap gains.
    int auto_unroll() const {
        if (knobs.unroll && *knobs.unroll >= 1 && *knobs.unroll <= 8) return *knobs.unroll;
        if (pixel_fetches == 0) return 1;
        return pixel_stmts <= 64 ? 4 : pixel_stmts <= 400 ? 2 : 1;
    }
    // Columns of a workgroup's 256 work-items.  16 x 16 keeps the gathers of a distortion local in both directions;
    // a body that is little more than its fetch (a copy, a scale, a flip) streams rows, and a wave that covers
    // 64 pixels of one row reads and writes whole cache lines (same A/B: Ident 0.204 -> 0.187 ms, Pond 0.673 -> 0.684).
    int auto_tile_w() const { return pixel_fetches >= 1 && pixel_stmts <= 12 ? 64 : 16; }

    void find_natives(Block &b, int loop_depth = 0) {
        for (Stmt *s : b) {
            if (s->kind == Stmt::Assign) {
                bool native = (s->rhs.kind == Rhs::Closure && s->rhs.filter->kind == Filter::Native) ||
                              (s->rhs.kind == Rhs::Op && !strcmp(s->rhs.op->cname, "RENDER"));
                if (native) {
                    NativeCall nc;
                    nc.func = s->rhs.kind == Rhs::Closure ? s->rhs.filter->native_func : "RENDER";
                    for (const Primary &p : s->rhs.args) nc.arg_types.push_back(p.type());
                    nc.in_loop = loop_depth > 0;
                    native_index[s] = (int)ks.natives.size();
                    ks.natives.push_back(nc);
                }
            } else if (s->kind == Stmt::If) {
                find_natives(s->then_, loop_depth);
                find_natives(s->else_, loop_depth);
            } else if (s->kind == Stmt::While)
                find_natives(s->body, loop_depth + 1);
        }
    }

    // ---- statement printing ------------------------------------------------------------------
    void phis(Block &list, int branch, Slice sl, const std::string &ind) {
        auto src = [&](const Stmt *p) -> const Rhs & { return branch == 0 ? p->rhs : p->rhs2; };
        auto src_value = [&](const Stmt *p) { return src(p).kind == Rhs::Prim && src(p).prim.kind == Primary::Val ? src(p).prim.value : nullptr; };
        std::vector<Stmt *> mine;
        std::set<Value *> targets;
        for (Stmt *p : list)
            if (p->kind == Stmt::Phi && (sl == PROLOGUE ? p->hoisted : p->in_pixel) && src_value(p) != p->lhs) { mine.push_back(p); targets.insert(p->lhs); }
        // phis are parallel copies: if a source is the target of another copy in the
        // list, go through temporaries
        bool hazard = false;
        for (Stmt *p : mine) hazard = hazard || targets.count(src_value(p)) > 0;
        if (!hazard) {
            for (Stmt *p : mine) out << ind << vname(p->lhs) << " = " << rhs(src(p), sl, p, p->lhs->var) << ";\n";
            return;
        }
        out << ind << "{\n";
        for (size_t i = 0; i < mine.size(); ++i)
            out << ind << "  " << ctype(mine[i]->lhs->var) << " pc" << i << " = "
                << rhs(src(mine[i]), sl, mine[i], mine[i]->lhs->var) << ";\n";
        for (size_t i = 0; i < mine.size(); ++i) out << ind << "  " << vname(mine[i]->lhs) << " = pc" << i << ";\n";
        out << ind << "}\n";
    }

    // sin(v) and cos(v) of the same float value in one block (toXY of an `ra` filter): evaluated
    // together by mmf_sincos_f32 -- one argument reduction -- at the first of the two statements.
    static bool is_sin_or_cos(const Stmt *s, bool *is_sin) {
        if (s->kind != Stmt::Assign || s->rhs.kind != Rhs::Op || s->rhs.args.size() != 1) return false;
        const char *cn = s->rhs.op->cname;
        if (strcmp(cn, "sin") && strcmp(cn, "cos")) return false;
        if (!s->lhs || s->lhs->var->type != Ty::Float || s->rhs.args[0].type() != Ty::Float || s->rhs.args[0].kind != Primary::Val)
            return false;
        *is_sin = !strcmp(cn, "sin");
        return true;
    }
    void join_sincos(Block &b) {      // (the pixel slice's)
        for (size_t i = 0; i < b.size(); ++i) {
            bool sin_i, sin_j;
            Stmt *si = b[i];
            if (!si->in_pixel || sincos_role.count(si) || !is_sin_or_cos(si, &sin_i)) continue;
            for (size_t j = i + 1; j < b.size(); ++j) {
                Stmt *sj = b[j];
                if (!sj->in_pixel || sincos_role.count(sj) || !is_sin_or_cos(sj, &sin_j)) continue;
                if (sin_j == sin_i || sj->rhs.args[0].value != si->rhs.args[0].value) continue;
                sincos_role[si] = SinCosRole{sincos_ids, true};
                sincos_role[sj] = SinCosRole{sincos_ids, false};
                ++sincos_ids;
                break;
            }
        }
    }

    void stmts(Block &b, Slice sl, const std::string &ind) {
        if (opt.fast_math_exact && sl == PIXEL && sincos_scanned.insert(&b).second) join_sincos(b);
        for (Stmt *s : b) {
            bool mine = sl == PROLOGUE ? s->hoisted : sl == ROWS ? s->in_row : s->in_pixel;
            if (!mine) continue;
            switch (s->kind) {
                case Stmt::Assign: {
                    auto sc = sl == PIXEL ? sincos_role.find(s) : sincos_role.end();
                    if (sc != sincos_role.end()) {
                        const std::string t = "mm_sc" + std::to_string(sc->second.id);
                        if (sc->second.first)
                            out << ind << "const mmf_sincos_t " << t << " = mmf_sincos_f32(" << prim(s->rhs.args[0], sl) << ");\n";
                        out << ind << vname(s->lhs) << " = " << t << (!strcmp(s->rhs.op->cname, "sin") ? ".s" : ".c") << ";\n";
                        break;
                    }
                    out << ind << vname(s->lhs) << " = " << rhs(s->rhs, sl, s, s->lhs->var) << ";\n";
                    break;
                }
                case Stmt::If:
                    out << ind << "if (" << rhs(s->cond, sl, s, nullptr) << ") {\n";
                    stmts(s->then_, sl, ind + "  ");
                    phis(s->phis, 0, sl, ind + "  ");
                    out << ind << "} else {\n";
                    stmts(s->else_, sl, ind + "  ");
                    phis(s->phis, 1, sl, ind + "  ");
                    out << ind << "}\n";
                    break;
                case Stmt::While: {
                    // a loop of both slices whose calls the prologue numbers: the pixel slice starts counting where the
                    // prologue stood when it entered the loop
                    auto db = dual_base_off.find(s);
                    if (db != dual_base_off.end() && sl == PROLOGUE)
                        out << ind << "*(int *)(XY + " << db->second << ") = ((const int *)(XY + " << ks.native_ctr_offset << "))[1];\n";
                    if (db != dual_base_off.end() && sl == PIXEL)
                        out << ind << "mm_dyn_ctr = *(const int *)(XY + " << db->second << ");\n";
                    phis(s->phis, 0, sl, ind);
                    out << ind << "while (" << rhs(s->cond, sl, s, nullptr) << ") {\n";
                    stmts(s->body, sl, ind + "  ");
                    phis(s->phis, 1, sl, ind + "  ");
                    out << ind << "}\n";
                    break;
                }
                default: break;
            }
        }
    }

    // `null_images`: image handles start as the null image -- in the prologue, whose every transferred value is stored at
    // the end whether or not the branch that assigns it ran (the pixel kernel loads the descriptors of transferred images
    // up front)
    void decls(const std::vector<Value *> &defs, const std::string &ind, bool null_images = false) {
        std::set<Value *> seen;
        for (Value *v : defs) {
            if (v->index < 0 || !seen.insert(v).second) continue;
            out << ind << ctype(v->var) << " " << vname(v) << (null_images && v->var->type == Ty::Image ? " = mm_null_image()" : "") << ";\n";
        }
    }

    // The clip variant (mm_*_clip, one launch for many frames) is this same text with the kernels' heads replaced: the
    // spans of `out` that differ are recorded while the text is emitted, so every body statement is emitted once, for both.
    void emit(const std::string &text, const std::string &clip_text) {      // `text`, and what stands in its place in the clip variant
        const size_t begin = (size_t)out.tellp();
        out << text;
        ks.clip_splices.push_back({begin, (size_t)out.tellp(), clip_text});
    }

    // Follows plain copies (and phis-free assignments of a primary) to the defining statement.
    static const Stmt *def_through_copies(const Primary &p) {
        const Primary *q = &p;
        for (int guard = 0; guard < 64; ++guard) {
            if (q->kind != Primary::Val || !q->value->def) return nullptr;
            const Stmt *d = q->value->def;
            if (d->kind != Stmt::Assign) return nullptr;
            if (d->rhs.kind == Rhs::Prim) { q = &d->rhs.prim; continue; }
            return d;
        }
        return nullptr;
    }
    // The filter whose pixel is nothing but the result of native call k sampled at the pixel's own
    // coordinates -- `soft = gaussian_blur(in, ...); soft(xy)`, examples/Blur/Gaussian Blur.mm.  The
    // host may then let the native filter's last kernel write the output pixels itself (when the
    // sample positions are the pixel centres, which it checks) and skip the pixel kernel.
    int find_direct_native() const {
        const Stmt *fetch = nullptr;
        for (int i = 0; i < 4; ++i) {
            if (!code.result[i]) return -1;
            const Stmt *d = def_through_copies(Primary::V(code.result[i]));
            if (!d || d->rhs.kind != Rhs::Op || strcmp(d->rhs.op->cname, "TUPLE_NTH") || d->rhs.args.size() != 2 ||
                d->rhs.args[1].kind != Primary::IntConst || d->rhs.args[1].i != i)
                return -1;
            const Stmt *t = def_through_copies(d->rhs.args[0]);
            if (!t || (fetch && t != fetch)) return -1;
            fetch = t;
        }
        if (fetch->rhs.kind != Rhs::Op || strcmp(fetch->rhs.op->cname, "ORIG_VAL") || fetch->rhs.args.size() < 3) return -1;
        const Stmt *dx = def_through_copies(fetch->rhs.args[0]), *dy = def_through_copies(fetch->rhs.args[1]);
        if (!dx || dx->rhs.kind != Rhs::Internal || dx->rhs.internal != "x") return -1;
        if (!dy || dy->rhs.kind != Rhs::Internal || dy->rhs.internal != "y") return -1;
        const Stmt *img = def_through_copies(fetch->rhs.args[2]);
        auto it = img ? native_index.find(img) : native_index.end();
        return it == native_index.end() || ks.natives[it->second].in_loop ? -1 : it->second;
    }

    // ---- the per-row slice ------------------------------------------------------------------
    // The reference evaluates code that depends on y alone once per row (its "x-const" slice, new_template.c.in:251-253,
    // compiler.c:4550-4611).  Here: top-level assignments of the pixel slice whose operands are literals, frame constants,
    // the row coordinate or other such values form the row slice -- when it contains a library call (everything else is
    // cheaper to recompute per pixel than to load) -- and a kernel of its own, mm_rows, evaluates it once per row of the
    // launch; the pixel kernel reads the values it needs from mm_args.rowtab like it reads y from ytab.
    static bool row_scalar(Ty t) { return t == Ty::Int || t == Ty::Float || t == Ty::Complex; }
    static bool row_expensive(const char *cn) {
        static const char *cheap[] = {"fabs", "floor", "ceil", "crealf", "cimagf"};
        for (const char *c : cheap) if (!strcmp(cn, c)) return false;
        return std::islower((unsigned char)cn[0]) || !strncmp(cn, "ELL_", 4) || !strcmp(cn, "GAMMA");
    }
    void find_row_slice() {
        if (fn_root || in_function || knobs.no_row_slice) return;
        if (opt.variant()) {
            // the second generation from this code: the slice is what the first run marked (it moved those statements
            // out of the pixel slice, so the search below would not find them again), its table in the same order
            std::vector<Value *> defs;
            std::set<Value *> used;
            collect_values(code.body, PIXEL, defs, used);
            for (int i = 0; i < 4; ++i) used.insert(code.result[i]);
            for (Stmt *s : code.body)
                if (s->kind == Stmt::Assign && s->in_row && used.count(s->lhs)) row_transfer.push_back(s->lhs);
            ks.row_values = (int)row_transfer.size();
            if (ks.row_values > 0) ks.rows_name = "mm_rows";
            return;
        }
        std::vector<Stmt *> cand;
        std::set<const Value *> rows;
        auto operand_ok = [&](const Primary &p) {
            return p.kind != Primary::Val || p.value->index < 0 || p.value->hoisted || rows.count(p.value) > 0;
        };
        for (Stmt *s : code.body) {           // top level only: no control flow in the row slice
            if (s->kind != Stmt::Assign || !s->in_pixel || s->hoisted || !row_scalar(s->lhs->var->type)) continue;
            const Rhs &r = s->rhs;
            bool ok = false;
            if (r.kind == Rhs::Internal) ok = r.internal == "y";
            else if (r.kind == Rhs::Prim) ok = operand_ok(r.prim) && r.prim.kind == Primary::Val && rows.count(r.prim.value);
            else if (r.kind == Rhs::Op && r.op->pure) {
                ok = true;
                bool any_row = false;
                for (const Primary &p : r.args) {
                    ok = ok && operand_ok(p) && (p.kind != Primary::Val || p.value->index < 0 || row_scalar(p.value->var->type));
                    any_row = any_row || (p.kind == Primary::Val && rows.count(p.value));
                }
                ok = ok && any_row && strncmp(r.op->cname, "USERVAL_", 8) != 0;
            }
            if (!ok) continue;
            cand.push_back(s);
            rows.insert(s->lhs);
        }
        // what the pixel code reads must travel as a 32-bit word: a complex row value that is used per pixel goes back to
        // the pixel slice, and with it whatever was computed from it
        std::set<Value *> used;      // by the pixel slice that is left
        for (bool changed = true; changed;) {
            changed = false;
            for (Stmt *s : cand) s->in_pixel = !rows.count(s->lhs);
            std::vector<Value *> defs;
            used.clear();
            collect_values(code.body, PIXEL, defs, used);
            for (int i = 0; i < 4; ++i) used.insert(code.result[i]);
            for (Stmt *s : cand) {
                if (!rows.count(s->lhs)) continue;
                bool drop = used.count(s->lhs) && s->lhs->var->type == Ty::Complex;
                if (s->rhs.kind == Rhs::Prim) drop = drop || !rows.count(s->rhs.prim.value);
                for (const Primary &p : s->rhs.args)
                    drop = drop || (p.kind == Primary::Val && p.value->index >= 0 && !p.value->hoisted && !rows.count(p.value));
                if (drop) { rows.erase(s->lhs); changed = true; }
            }
        }
        bool expensive = false;
        for (Stmt *s : cand)
            expensive = expensive || (rows.count(s->lhs) && s->rhs.kind == Rhs::Op && row_expensive(s->rhs.op->cname));
        for (Stmt *s : cand) if (rows.count(s->lhs) && used.count(s->lhs)) row_transfer.push_back(s->lhs);
        if (!expensive || row_transfer.empty() || row_transfer.size() > 24) {      // not worth a kernel and a table
            for (Stmt *s : cand) s->in_pixel = true;
            row_transfer.clear();
            return;
        }
        for (Stmt *s : cand)
            if (rows.count(s->lhs)) { s->in_row = true; s->in_pixel = false; s->lhs->row_const = true; }
        ks.row_values = (int)row_transfer.size();
        ks.rows_name = "mm_rows";
    }
    // the frame constants a kernel reads, from where the prologue left them (`only`: those of them that it uses)
    void transfer_loads(const std::set<Value *> *only, const char *ind = "  ") {
        for (Value *v : transfer_order)
            if (!only || only->count(v))
                out << ind << "const " << ctype(v->var) << " " << vname(v) << " = *(const " << ctype(v->var) << " *)(XY + " << transfer_off[v] << ");\n";
    }
    // the row values a pixel of row `row` needs, from the table mm_rows filled
    void row_loads(const std::string &ind, const char *row) {
        for (size_t k = 0; k < row_transfer.size(); ++k) {
            Value *v = row_transfer[k];
            const std::string at = "A.rowtab[" + std::to_string(k) + " * A.num_rows + " + row + "]";
            out << ind << "const " << ctype(v->var) << " " << vname(v) << " = "
                << (v->var->type == Ty::Int ? "__float_as_int(" + at + ")" : at) << ";\n";
        }
    }

    void analyze_and_layout() {
        find_natives(code.body);
        ks.native_sites = (int)ks.natives.size();
        // A call site inside a loop makes one call per iteration, each with a result of its own (the next iteration, or
        // the code behind the loop, may read it): such calls are numbered as the prologue makes them and recorded in
        // dynamic entries behind the sites'.  The host runs all recorded calls in the order they were made.
        bool any_in_loop = false;
        for (const NativeCall &nc : ks.natives) any_in_loop = any_in_loop || nc.in_loop;
        NativeCall dynamic_entry;
        dynamic_entry.dynamic = true;
        if (any_in_loop) ks.natives.insert(ks.natives.end(), MM_NATIVE_DYN_CALLS, dynamic_entry);
        ks.direct_native = find_direct_native();
        find_row_slice();
        collect_values(code.body, PROLOGUE, pro_defs, pro_uses);
        collect_values(code.body, PIXEL, pix_defs, pix_uses);
        collect_values(code.body, ROWS, row_defs, row_uses);
        for (Value *v : row_uses) if (v && v->hoisted) pix_uses.insert(v);      // frame constants the row slice reads travel in XY too
        for (int i = 0; i < 4; ++i) pix_uses.insert(code.result[i]);
        std::set<Value *> pix_def_set(pix_defs.begin(), pix_defs.end());
        for (Value *v : row_transfer) pix_def_set.insert(v);                    // defined (loaded) per pixel
        int off = 0;
        // native call records first (fixed layout the host can parse)
        for (NativeCall &nc : ks.natives) {
            nc.record_offset = off;
            off += MM_NATIVE_REC_BYTES;
        }
        if (!ks.natives.empty()) {
            ks.native_ctr_offset = off;
            off += 16;
        }
        for (Value *v : pro_defs) {
            if (!pix_uses.count(v) || pix_def_set.count(v) || transfer_off.count(v)) continue;
            int sz = type_size(v->var);
            int align = sz >= 8 ? 8 : 4;
            off = (off + align - 1) / align * align;
            transfer_off[v] = off;
            transfer_order.push_back(v);
            off += sz;
        }
        if (ks.native_sites < (int)ks.natives.size())      // the outermost loops of both slices: loops inside them go on counting
            each_stmt(code.body, [&](const Stmt *s) {
                if (s->kind != Stmt::While || !s->hoisted || !s->in_pixel) return true;
                off = (off + 3) / 4 * 4;
                dual_base_off[s] = off;
                off += 4;
                return false;
            });
        ks.xy_bytes = (off + 15) / 16 * 16;
        if (ks.xy_bytes == 0) ks.xy_bytes = 16;
        ks.has_prologue = !pro_defs.empty();
        // a value used by the pixel slice must be defined there or transferred
        for (Value *v : pix_uses)
            if (v && v->index >= 0 && !pix_def_set.count(v) && !transfer_off.count(v))
                throw CompileError("internal: value " + vname(v) + " used in the pixel kernel but defined nowhere");
        pixel_stats(code.body, pixel_stmts, pixel_fetches);
    }

    // ---- the translation unit, top to bottom ----
    void run() {
        analyze_and_layout();
        emit_options();
        emit_preludes();
        emit_functions();
        if (pair) pair->emit_helpers();
        emit_prologue_kernel();
        if (ks.row_values > 0) emit_rows_kernel();
        if (opt.sampled) emit_sampled_pixel_kernel();
        else if (opt.shutter) emit_shutter_pixel_kernel();
        else emit_pixel_kernel();
        ks.source = out.str();
        if (opt.variant()) {      // the prologue and the per-row slice in their clip form; the pixel kernel has no other
            std::string text, key;
            clip_kernel_source(ks, &text, &key);
            ks.source = std::move(text);
            ks.clip_splices.clear();
        }
        ks.key = text_key(ks.source);
        ks.wrapping_ints = opt.edge_x >= 2 || opt.edge_y >= 2;      // REFLECT, ROTATE (KernelSource::wrapping_ints)
    }

    // the compile-time options as #defines; decides the workgroup shape, the unroll factor and pair mode
    void emit_options() {
        int tw = knobs.tile_w.value_or(opt.tile_w);      // experiments (tools/ab_unroll.sh)
        if (tw != 8 && tw != 16 && tw != 32 && tw != 64 && tw != 128 && tw != 256) tw = auto_tile_w();
        ks.tile_w = tw;
        ks.tile_h = 256 / tw;
        // non-temporal output stores keep the frame from displacing the *input* in the caches: for kernels that fetch
        // (a kernel that reads nothing gains nothing, and its 64-byte row segments then reach memory uncombined:
        // Mandelbrot 8192^2 wrote 347 MB instead of 268 MB in the WRITE_SIZE counter, same time)
        out << "#define MM_NT_STORE " << knobs.nt_store.value_or(pixel_fetches > 0) << "\n";
        // Workgroup -> tile order.  Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  Giving every
        // XCD one contiguous band of tiles (1) lets neighbouring gathers share an L2 -- and makes every XCD's share of
        // the work depend on *where* in the frame the work is: the rows of a Mandelbrot frame that cross the set iterate
        // 2-3 times longer than its top and bottom rows, Droste's level loop runs for some regions only, and the XCDs
        // that own the cheap bands idle while the others finish (first seen as two processes sharing the GPU rendering
        // 20 % more frames than one: the idle XCDs took the other process's workgroups).  Tiles in dispatch order (0)
        // spread every region over all XCDs but put horizontal neighbours on different L2s (Pond fetched 2.8x its
        // input).  The default (2) deals runs of about one tile row to the XCDs in turn: balanced like (0), and a row's
        // tiles share an L2 like in (1).  A/B at 8192^2, ms for orders 0 / 1 / 2 (tools/ab_xcd_order.sh,
        // profiles/r03_ab_xcd_order.txt): Mandelbrot 0.209 / 0.263 / 0.201, Droste 0.860 / 1.217 / 0.855 (NoTransparency=1:
        // 0.853 / 0.905 / 0.852), Pond 0.569 / 0.567 / 0.556, Ident 0.140 / 0.133 / 0.133.
        ks.xcd_order = knobs.xcd_order.value_or(2);
        out << "#define MM_XCD_ORDER " << ks.xcd_order << "\n";
        if (knobs.pair_masks) out << "#define MM_PAIR_MASKS " << *knobs.pair_masks << "\n";
        if (knobs.no_same_taps) out << "#define MM_NO_SAME_TAPS 1\n";      // A/B switches
        if (knobs.no_outside_shortcut) out << "#define MM_NO_OUTSIDE_SHORTCUT 1\n";
        out << "#define MM_INTERSAMPLE " << opt.intersample << "\n";
        out << "#define MM_SUPERSAMPLING " << opt.supersampling << "\n";
        out << "#define MM_EDGE_X " << opt.edge_x << "\n#define MM_EDGE_Y " << opt.edge_y << "\n";
        if (opt.pixel_inc > 1) out << "#define MM_PIXEL_INC " << opt.pixel_inc << "\n";
        if (opt.deep_inputs) out << "#define MM_DEEP_INPUTS 1\n";
        out << "#define MM_TILE_W " << ks.tile_w << "\n#define MM_TILE_H " << ks.tile_h << "\n";
        ks.unroll = opt.unroll > 0 ? opt.unroll : auto_unroll();
        // pair mode (row values are per pixel of a pair; a native call is not arithmetic)
        if (opt.variant()) ks.unroll = 1;      // (single-pixel shape, general fetch: emit_shutter_pixel_kernel)
        else if (opt.unroll <= 0 && !knobs.unroll && ks.row_values == 0 && ks.natives.empty())
            pair = make_pair_mode(PairEnv{out, code, opt, knobs, pix_defs, pixel_stmts, pixel_fetches,
                                          [this](const Primary &p) { return prim(p, PIXEL); },
                                          [this](const Stmt *s) { return rhs(s->rhs, PIXEL, s, s->lhs->var); },
                                          [this](const Value *v) { return value_visible(v, PIXEL); },
                                          [this](const std::string &text, const std::string &clip_text) { emit(text, clip_text); }});
        if (pair) ks.unroll = 2;
        ks.pair_mode = pair != nullptr;
        ks.pair_exit = pair && pair->exit_driven();
        out << "#define MM_UNROLL " << ks.unroll << "\n";
        out << "#define MM_NATIVE_REC_BYTES " << (int)MM_NATIVE_REC_BYTES << "\n#define MM_NATIVE_DYN_CALLS " << (int)MM_NATIVE_DYN_CALLS << "\n";
    }

    // the math and device preludes, and the helper text every kernel of the translation unit may use
    void emit_preludes() {
        // float-argument sin/cos (mm_fastmath.h), the same text the host verifier compiles; it
        // precedes the device prelude, whose complex functions use mmf_sincos_d
        out << "#define MMF_FN static __device__ __forceinline__\n#define MMF_CONST_TABLE static __device__ const\n"
               "#define MMG_FN static __device__\n"
               "#define MMF_FMA(a, b, c) __builtin_fma((a), (b), (c))\n#define MMF_RINT(a) __builtin_rint((a))\n"
               "#define MMF_FABSF(a) __builtin_fabsf((a))\n#define MMF_FABS(a) __builtin_fabs((a))\n"
               "#define MMF_SIN_SLOW(a) sin((a))\n#define MMF_COS_SLOW(a) cos((a))\n"
               "#define MMF_LDEXP(a, e) __builtin_ldexp((a), (e))\n#define MMF_EXP_SLOW(a) exp((a))\n#define MMF_LOG_SLOW(a) log((a))\n"
               "#define MMF_POW_SLOW(a, b) pow((a), (b))\n"
               "#define MMF_ASINH_SLOW(a) asinh((a))\n#define MMF_ACOSH_SLOW(a) acosh((a))\n"
               "#define MMF_SQRT(a) __builtin_sqrt((a))\n#define MMF_HYPOT_SLOW(a, b) hypot((a), (b))\n"
               // mm_glibcf.h (glibc's float algorithms for the complex ops); float sqrt / division are the correctly
               // rounded device ones, double sqrt is the compiler's correctly rounded expansion
               "#define MMQ_FN static __device__ __forceinline__\n#define MMQ_TABLE static __device__ const\n"
               "#define MMQ_FMA(a, b, c) __builtin_fma((a), (b), (c))\n#define MMQ_SQRT(a) sqrt((a))\n"
               "#define MMQ_SQRTF(a) sqrtf((a))\n"
            << device_fastmath_prelude() << "\n";
        out << (opt.deep_inputs ? device_prelude() : plain_device_prelude().c_str()) << "\n";
        bool noise = uses_noise(code.body);
        for (auto &fn : (fn_root ? fn_root : &code)->functions) noise = noise || uses_noise(fn->body);
        if (noise) {
            if (!noise_table_text())
                throw CompileError("the noise builtins need libnoise's gradient table, which was not available when this "
                                   "library was built (see tools/extract_noise_table.py)");
            out << noise_table_text() << device_noise_prelude() << "\n";
        }
        out << R"(
MM_DEV mm_image mm_closure_image(const mm_args &A, int closure_id) {
    mm_image im; im.idx = closure_id < 0 ? -1 : -2 - closure_id; im.pw = A.img_width; im.ph = A.img_height;
    im.xf = im.yf = 1.0f; im.resized = 0; return im;
}
struct mm_narg_t { int kind; int i; float f; mm_image img; };
MM_DEV mm_narg_t mm_narg(int v) { mm_narg_t a; a.kind = 0; a.i = v; a.f = (float)v; a.img = mm_null_image(); return a; }
MM_DEV mm_narg_t mm_narg(float v) { mm_narg_t a; a.kind = 1; a.i = (int)v; a.f = v; a.img = mm_null_image(); return a; }
MM_DEV mm_narg_t mm_narg(double v) { return mm_narg((float)v); }
MM_DEV mm_narg_t mm_narg(mm_image v) { mm_narg_t a; a.kind = 2; a.i = v.idx; a.f = 0.0f; a.img = v; return a; }
// Records a native-filter call for the host (which runs the filter's kernels between
// the prologue and the pixel kernel) and returns the handle of its result float map.
// ctr[0] counts the calls of this frame in the order they are made (the host runs them in that order).
MM_DEV mm_image mm_native_call(const mm_args &A, char *rec, int *ctr, int k, int nargs, mm_narg_t a0, mm_narg_t a1, mm_narg_t a2, mm_narg_t a3) {
    int *hdr = (int *)rec;
    hdr[0] = 1; hdr[1] = k; hdr[2] = nargs; hdr[3] = ctr[0]++;
    mm_narg_t *args = (mm_narg_t *)(rec + 16);
    args[0] = a0; args[1] = a1; args[2] = a2; args[3] = a3;
    mm_image im; im.idx = A.native_slot_base + k; im.pw = A.render_width; im.ph = A.render_height;
    im.xf = im.yf = 1.0f; im.resized = 0;
    return im;
}
// The same for a call site inside a loop: every call takes the next of the MM_NATIVE_DYN_CALLS dynamic entries behind
// the `sites' call sites (record, result slot); one call too many raises ctr[2] and the host refuses the frame.
MM_DEV mm_image mm_native_call_in_loop(const mm_args &A, char *dyn, int *ctr, int site, int sites, int nargs, mm_narg_t a0, mm_narg_t a1,
                                       mm_narg_t a2, mm_narg_t a3) {
    int n = ctr[1]++;
    if (n >= MM_NATIVE_DYN_CALLS) { ctr[2] = 1; n = MM_NATIVE_DYN_CALLS - 1; }
    mm_image im = mm_native_call(A, dyn + n * MM_NATIVE_REC_BYTES, ctr, site, nargs, a0, a1, a2, a3);
    im.idx = A.native_slot_base + sites + n;
    return im;
}
// (float) frame column / row of the pixel being evaluated (render_image's per-pixel loop, builtins.c:324-333)
#define __colF ((float)(col + A.region_x))
#define __rowF ((float)(rl + A.first_row))
#define MM_INTERNALS \
    const float t = A.t; const float R = A.R; const int frame = A.frame; \
    const int __canvasPixelW = A.img_width, __canvasPixelH = A.img_height; \
    const int __renderPixelW = A.render_width, __renderPixelH = A.render_height; \
    (void)t; (void)R; (void)frame; (void)__canvasPixelW; (void)__canvasPixelH; (void)__renderPixelW; (void)__renderPixelH;
)";
        if (ks.native_sites < (int)ks.natives.size())      // (only kernels with in-loop native calls: the others' text, and cache keys, stay as they were)
            out << R"(// The pixel slice's side of a loop that runs in both slices: its n-th call from an in-loop site is the prologue's n-th.
MM_DEV mm_image mm_native_result_in_loop(const mm_args &A, int &n, int sites) {
    mm_image im; im.idx = A.native_slot_base + sites + (n < MM_NATIVE_DYN_CALLS ? n : MM_NATIVE_DYN_CALLS - 1); ++n;
    im.pw = A.render_width; im.ph = A.render_height; im.xf = im.yf = 1.0f; im.resized = 0;
    return im;
}
)";
    }

    // filter_$name of every filter that is called at run time.  The reference's are ordinary recursive C functions;
    // a GPU kernel wants a stack bound it can prove, so each is a template on the call depth: depth D calls depth
    // D + 1, and depth MM_MAX_CALL_DEPTH returns the zero tuple without evaluating anything -- the call graph is
    // a finite DAG, the compiler computes the exact stack need, nothing can overflow.  (A recursion deeper than
    // that is cut off; the reference would keep going until its C stack overflows.)
    void emit_functions() {
        FilterCode &root = fn_root ? *fn_root : code;
        if (root.functions.empty()) return;
        out << "#ifndef MM_MAX_CALL_DEPTH\n#define MM_MAX_CALL_DEPTH " << knobs.max_call_depth.value_or(16)
            << "\n#endif\n"
               "struct mm_uvarg { int i; float f; color_t c; mm_image img; };\n";
        auto head = [](size_t k) {
            return "template <int MM_D> __device__ __noinline__ mm_tup<4> mm_filter_" + std::to_string(k) +
                   "(const mm_args &A, const mm_uvarg *UV, float x, float y, float t, int col, int rl, unsigned &mm_rand_ctr)";
        };
        for (size_t k = 0; k < root.functions.size(); ++k) out << head(k) << ";\n";
        for (size_t k = 0; k < root.functions.size(); ++k) {
            FilterCode &fn = *root.functions[k];
            Generator g(fn, opt, knobs);
            g.fn_root = &root;
            g.in_function = true;
            std::vector<Value *> defs;
            std::set<Value *> uses;
            g.collect_values(fn.body, PIXEL, defs, uses);
            out << "// filter_" << (fn.filter ? fn.filter->name : "") << "\n" << head(k) << " {\n"
                   "  mm_tup<4> rt;\n  rt.v[0] = rt.v[1] = rt.v[2] = rt.v[3] = 0.0f;\n"
                   "  if constexpr (MM_D >= MM_MAX_CALL_DEPTH) { return rt; } else {\n"
                   "  const float R = A.R; const int frame = 0;      // new_template.c.in:379: filter_$name has `int frame = 0`\n"
                   "  const int __canvasPixelW = A.img_width, __canvasPixelH = A.img_height;\n"
                   "  const int __renderPixelW = A.render_width, __renderPixelH = A.render_height;\n"
                   "  (void)R; (void)frame; (void)__canvasPixelW; (void)__canvasPixelH; (void)__renderPixelW; (void)__renderPixelH;\n";
            g.decls(defs, "  ");
            g.stmts(fn.body, PIXEL, "  ");
            out << g.out.str();
            for (int i = 0; i < 4; ++i) out << "  rt.v[" << i << "] = " << g.prim(Primary::V(fn.result[i]), PIXEL) << ";\n";
            out << "  return rt;\n  }\n}\n";
        }
    }

    // ---- prologue ----
    void emit_prologue_kernel() {
        ks.prologue_uses_time = hoisted_uses_time(code.body);
        ks.prologue_name = "mm_prologue";
        ks.pixel_name = "mm_pixels";
        // all lanes: the coordinate tables.  They depend on the geometry alone: in a clip (one grid row per frame of the
        // batch) the first row writes them
        auto tables = [](const std::string &first) {
            return "  {\n    const int gid = blockIdx.x * 256 + threadIdx.x;\n"
                   "    if (" + first + "gid < A.region_width) A.xtab[gid] = CALC_VIRTUAL_X(gid + A.region_x, A.frame_render_width, A.sampling_offset_x);\n"
                   "    if (" + first + "gid < A.num_rows) A.ytab[gid] = CALC_VIRTUAL_Y(A.first_row + gid, A.frame_render_height, A.sampling_offset_y);\n"
                   "    if (gid != 0) return;\n  }\n";
        };
        // the sampled variant: besides them one x table per grid column and one y table per grid row, the same expressions
        // at the offsets of S.offs (mm_sample_grid.h on the host) -- the bits a render at that sampling offset computes
        const std::string sampled_tables =
            "  {\n    const int gid = blockIdx.x * 256 + threadIdx.x;\n"
            "    if (fi == 0 && gid < A.region_width) {\n"
            "      A.xtab[gid] = CALC_VIRTUAL_X(gid + A.region_x, A.frame_render_width, A.sampling_offset_x);\n"
            "      for (int mm_a = 0; mm_a < S.gx; ++mm_a)\n"
            "        S.xtabs[mm_a * A.region_width + gid] = CALC_VIRTUAL_X(gid + A.region_x, A.frame_render_width, S.offs[mm_a]);\n"
            "    }\n"
            "    if (fi == 0 && gid < A.num_rows) {\n"
            "      A.ytab[gid] = CALC_VIRTUAL_Y(A.first_row + gid, A.frame_render_height, A.sampling_offset_y);\n"
            "      for (int mm_b = 0; mm_b < S.gy; ++mm_b)\n"
            "        S.ytabs[mm_b * A.num_rows + gid] = CALC_VIRTUAL_Y(A.first_row + gid, A.frame_render_height, S.offs[MM_SAMPLE_GRID_MAX + mm_b]);\n"
            "    }\n"
            "    if (gid != 0) return;\n  }\n";
        const std::string clip_head =
            opt.sampled ? std::string(clip_prelude()) + sampled_prelude() + KERNEL +
                              "mm_prologue_clip(mm_args A, char *XY, const mm_clip C, const mm_sampled S) {\n  MM_CLIP_ENTRY\n" + sampled_tables
                        : (ks.natives.empty() ? clip_prelude() : clip_prelude_natives()) + KERNEL +
                              "mm_prologue_clip(mm_args A, char *XY, const mm_clip C) {\n  MM_CLIP_ENTRY\n" + tables("fi == 0 && ");
        emit(KERNEL + "mm_prologue(mm_args A, char *XY) {\n" + tables(""), clip_head);
        out << "  MM_INTERNALS\n";
        if (!(fn_root ? fn_root : &code)->functions.empty()) out << "  const int col = 0, rl = 0; unsigned mm_rand_ctr = 0; (void)col; (void)rl; (void)mm_rand_ctr;\n";
        decls(pro_defs, "  ", true);
        if (!ks.natives.empty()) {      // no call recorded yet this frame
            for (const NativeCall &nc : ks.natives) out << "  *(int *)(XY + " << nc.record_offset << ") = 0;\n";
            out << "  { int *mm_ctr = (int *)(XY + " << ks.native_ctr_offset << "); mm_ctr[0] = mm_ctr[1] = mm_ctr[2] = mm_ctr[3] = 0; }\n";
        }
        stmts(code.body, PROLOGUE, "  ");
        for (Value *v : transfer_order)
            out << "  *(" << ctype(v->var) << " *)(XY + " << transfer_off[v] << ") = " << vname(v) << ";\n";
        out << "}\n\n";
    }

    // ---- rows kernel: the per-row slice, one lane per row of the launch ----
    void emit_rows_kernel() {
        emit(KERNEL + "mm_rows(mm_args A, const char *__restrict__ XY) {\n",
             KERNEL + "mm_rows_clip(mm_args A, const char *__restrict__ XY, const mm_clip C) {\n  MM_CLIP_ENTRY\n");
        out << "  const int rl = blockIdx.x * 256 + threadIdx.x;\n"
               "  if (rl >= A.num_rows) return;\n"
               "  MM_INTERNALS\n"
               "  const float y = A.ytab[rl];    // CALC_VIRTUAL_Y(first_row + rl, ...), by the prologue\n"
               "  (void)y;\n";
        transfer_loads(&row_uses);
        decls(row_defs, "  ");
        stmts(code.body, ROWS, "  ");
        for (size_t k = 0; k < row_transfer.size(); ++k) {
            Value *v = row_transfer[k];
            out << "  A.rowtab[" << k << " * A.num_rows + rl] = "
                << (v->var->type == Ty::Int ? "__int_as_float(" + vname(v) + ")" : vname(v)) << ";\n";
        }
        out << "}\n\n";
    }

    // ---- pixel kernel: its head, then one of the two shapes ----
    void emit_pixel_kernel() {
        // experiment hook: ask the register allocator for a minimum occupancy (waves per SIMD)
        if (knobs.waves_per_eu) out << "__attribute__((amdgpu_waves_per_eu(" << *knobs.waves_per_eu << "))) ";
        // (a clip's grid is padded in x to a multiple of 8, so that a workgroup's XCD is bid & 7 in every frame)
        emit(KERNEL + "mm_pixels(mm_args A, const char *__restrict__ XY) {\n",
             KERNEL + "mm_pixels_clip(mm_args A, const char *__restrict__ XY, const mm_clip C) {\n"
                      "  if ((int)blockIdx.x >= C.nwg) return;      // padding workgroup\n  MM_CLIP_ENTRY\n");
        out << "  MM_INTERNALS\n";
        emit_tile_order(true);
        transfer_loads(nullptr);
        // Large bodies keep the one-pixel-per-work-item shape: a pixel loop makes every frame
        // constant live across it in SGPRs (after the loop's first store the compiler may not
        // re-issue scalar loads), and Droste's ~60 of them spilled to VGPR lanes -- 1.7x slower.
        // Such kernels are compute-bound; the per-workgroup dispatch cost does not show.
        ks.single_pixel = knobs.single_pixel ? *knobs.single_pixel != 0 : pixel_stmts > 400 || transfer_order.size() > 24;
        if (ks.single_pixel) emit_single_pixel();
        else emit_pixel_loops();
    }

    // from the workgroup to its tile, column and first row (`both`: the text of mm_pixels and, as splices, of mm_pixels_clip;
    // else the clip form alone)
    void emit_tile_order(bool both) {
        out << R"(  // XCD-aware tile order (MM_XCD_ORDER, above): workgroups are dealt round-robin to the 8 XCDs; give each
  // XCD one contiguous band of tiles so neighbouring gathers share its L2 -- or, for a kernel that reads nothing,
  // take the tiles in dispatch order so that cheap and expensive regions of the frame are spread over all XCDs.
  const int tiles_x = (A.region_width + MM_TILE_W - 1) / MM_TILE_W;
)";
        const char *clip_nwg = "  const int nwg = C.nwg;      // the frame's workgroups (gridDim.x is padded)\n";
        if (both) emit("  const int nwg = gridDim.x;\n", clip_nwg);
        else out << clip_nwg;
        out << R"(  const int bid = blockIdx.x;
#if MM_XCD_ORDER == 1
  const int xcd = bid & 7, q = bid >> 3;
  const int per = nwg >> 3, rem = nwg & 7;
  const int swz = xcd * per + (xcd < rem ? xcd : rem) + q;
#elif MM_XCD_ORDER == 2
  // runs of C = 2^m consecutive tiles (m: one tile row or a little more) dealt to the XCDs in turn: neighbours in a row
  // share an L2 like in a band, and every XCD gets runs from all over the frame; the last partial round keeps dispatch order
  const int m = 32 - __builtin_clz((unsigned)(tiles_x > 1 ? tiles_x - 1 : 1));
  const int full = (nwg >> (m + 3)) << (m + 3);
  const int q = bid >> 3;
  const int swz = bid < full ? ((((q >> m) << 3) + (bid & 7)) << m) + (q & ((1 << m) - 1)) : bid;
#else
  const int swz = bid;
  (void)nwg;
#endif
  const int tile_y = A.tiles_magic ? (int)__umulhi((unsigned)swz, A.tiles_magic) : swz / tiles_x, tile_x = swz - tile_y * tiles_x;
  const int col = tile_x * MM_TILE_W + (threadIdx.x % MM_TILE_W);
  // a workgroup owns MM_TILE_W x (MM_TILE_H * A.ppt) pixels; each work-item walks A.ppt rows
  // MM_TILE_H apart, so wave start-up (kernarg / descriptor loads, tile arithmetic) and the
  // dispatcher's per-workgroup cost are paid once per A.ppt pixels
  const int row0 = tile_y * (MM_TILE_H * A.ppt) + (threadIdx.x / MM_TILE_W);   // row within this launch
  if (col >= A.region_width) return;
  const float x = A.xtab[col];   // CALC_VIRTUAL_X(col + region_x, ...), once per column
  (void)x;
)";
    }

    // single shape: one pixel per work-item
    void emit_single_pixel() {
        ks.unroll = 1;
        ks.pair_mode = false;
        out << "  const int rl = row0;   // A.ppt is 1 for this kernel (KernelSource::single_pixel)\n"
               "  if (rl >= A.num_rows) return;\n"
               "  const float y = A.ytab[rl];    // CALC_VIRTUAL_Y(first_row + rl, ...), once per row by the prologue\n"
               "  unsigned mm_rand_ctr = 0;      // RAND call number within this pixel\n"
               "  (void)y; (void)mm_rand_ctr;\n";
        if (!dual_base_off.empty())
            out << "  int mm_dyn_ctr = 0;            // in-loop native calls made so far by this pixel's copy of a loop of both slices\n";
        row_loads("  ", "rl");
        decls(pix_defs, "  ");
        stmts(code.body, PIXEL, "  ");
        out << "  mm_tup<4> rt;\n";
        for (int i = 0; i < 4; ++i) out << "  rt.v[" << i << "] = " << prim(Primary::V(code.result[i]), PIXEL) << ";\n";
        out << "  mm_store_pixel(A, rl, col, rt);\n}\n";
    }

    // ---- the shutter variant's pixel kernel (KernelOptions::shutter) ----
    // One work-item per output pixel of grid row fi, the single shape's body in a loop over the pixel's S.samples
    // sub-samples: sub-sample j is slot fi * S.samples + j of the batch -- its {t, frame} entry, its frame constants and
    // its row table, as mm_prologue_clip and mm_rows_clip left them.  What is summed is what mm_store_pixel would have
    // been handed for the sub-sample's float map; the sum's order and the product are mmhip_render_clip_shutter's.
    void emit_shutter_pixel_kernel() {
        if (!ks.natives.empty()) throw CompileError("the shutter variant is for filters without native calls");
        ks.single_pixel = true;
        ks.pair_mode = false;
        ks.pixel_name = "mm_pixels_shutter";
        out << shutter_prelude();
        if (knobs.waves_per_eu) out << "__attribute__((amdgpu_waves_per_eu(" << *knobs.waves_per_eu << "))) ";
        out << KERNEL
            << "mm_pixels_shutter(mm_args A, const char *__restrict__ XY, const mm_clip C, const mm_shutter S) {\n"
               "  if ((int)blockIdx.x >= C.nwg) return;      // padding workgroup\n"
               "  const int fi = blockIdx.y;                 // the output frame\n"
               "  A.out = (char *)A.out + (long long)fi * C.frame_stride;\n";
        emit_tile_order(false);
        out << "  const int rl = row0;   // A.ppt is 1 for this kernel\n"
               "  if (rl >= A.num_rows) return;\n"
               "  const float y = A.ytab[rl];    // CALC_VIRTUAL_Y(first_row + rl, ...), once per row by the prologue\n"
               "  (void)y;\n"
               "  const char *const mm_xy0 = XY;\n"
               "  float *const mm_rowtab0 = A.rowtab;\n"
               "  mm_tup<4> mm_acc;\n"
               "  mm_acc.v[0] = mm_acc.v[1] = mm_acc.v[2] = mm_acc.v[3] = 0.0f;\n"
               "#pragma unroll 1\n"
               "  for (int mm_j = 0; mm_j < S.samples; ++mm_j) {\n"
               "    const long long mm_slot = (long long)fi * S.samples + mm_j;\n"
               "    { const mm_clip_frame mm_cf = C.frames[mm_slot]; A.t = mm_cf.t; A.frame = mm_cf.frame; }\n"
               "    const char *__restrict__ XY = mm_xy0 + mm_slot * C.xy_stride;\n"
               "    if (mm_rowtab0) A.rowtab = mm_rowtab0 + mm_slot * C.rowtab_stride;\n"
               "    MM_INTERNALS\n"
               "    unsigned mm_rand_ctr = 0;      // RAND call number within this pixel: every sub-sample is a render of its own\n"
               "    (void)XY; (void)mm_rand_ctr;\n";
        transfer_loads(nullptr, "    ");
        row_loads("    ", "rl");
        decls(pix_defs, "    ");
        stmts(code.body, PIXEL, "    ");
        out << "    mm_tup<4> rt;\n";
        for (int i = 0; i < 4; ++i) out << "    rt.v[" << i << "] = " << prim(Primary::V(code.result[i]), PIXEL) << ";\n";
        out << "    if (mm_j == 0) mm_acc = rt;\n"
               "    else\n"
               "      for (int mm_c = 0; mm_c < 4; ++mm_c) mm_acc.v[mm_c] = mm_acc.v[mm_c] + rt.v[mm_c];\n"
               "  }\n"
               "  mm_tup<4> mm_m;\n"
               "  for (int mm_c = 0; mm_c < 4; ++mm_c) mm_m.v[mm_c] = mm_acc.v[mm_c] * S.inv_k;\n"
               "  mm_store_pixel(A, rl, col, mm_m);\n}\n";
    }

    // ---- the sampled variant's pixel kernel (KernelOptions::sampled) ----
    // mm_pixels_shutter's shape with a loop over the S.total = K * gx * gy sub-samples of a pixel: sub-sample s is
    // (j, b, a) with a fastest, decoded by counters.  j alone selects the slot fi * K + j ({t, frame} and the frame
    // constants); a and b select x and y, read from the per-offset tables mm_prologue_clip wrote -- entry col of table a,
    // entry rl of table b: a wave-uniform base (mm_xo, mm_yo advance by one table per step) and the lane's own index.
    // No per-row slice: its values follow y, and such filters take the maps path.
    void emit_sampled_pixel_kernel() {
        if (!ks.natives.empty()) throw CompileError("the sampled variant is for filters without native calls");
        if (ks.row_values > 0) throw CompileError("the sampled variant is for filters without a per-row slice");
        ks.single_pixel = true;
        ks.pair_mode = false;
        ks.pixel_name = opt.refine ? "mm_pixels_refine" : "mm_pixels_sampled";
        if (opt.refine) out << refine_prelude();
        if (knobs.waves_per_eu) out << "__attribute__((amdgpu_waves_per_eu(" << *knobs.waves_per_eu << "))) ";
        if (opt.refine) {
            // the refine variant: work-item i of grid row fi renders entry i of frame fi's list, whatever the tile order
            out << KERNEL
                << "mm_pixels_refine(mm_args A, const char *__restrict__ XY, const mm_clip C, const mm_sampled S, const mm_refine R) {\n"
                   "  const int fi = blockIdx.y;                 // the output frame\n"
                   "  const unsigned mm_i = blockIdx.x * 256u + threadIdx.x;\n"
                   "  if (mm_i >= R.counts[fi]) return;          // the launch covers the whole rectangle: the list may be shorter\n"
                   "  A.out = (char *)A.out + (long long)fi * C.frame_stride;\n"
                   "  const unsigned mm_e = R.list[(long long)fi * R.list_stride + mm_i];\n"
                   "  const int col = (int)(mm_e & 0xffffu), rl = (int)(mm_e >> 16);      // col | rl << 16, by the mask kernel\n";
        } else {
            out << KERNEL
                << "mm_pixels_sampled(mm_args A, const char *__restrict__ XY, const mm_clip C, const mm_sampled S) {\n"
                   "  if ((int)blockIdx.x >= C.nwg) return;      // padding workgroup\n"
                   "  const int fi = blockIdx.y;                 // the output frame\n"
                   "  A.out = (char *)A.out + (long long)fi * C.frame_stride;\n";
            emit_tile_order(false);
            out << "  const int rl = row0;   // A.ppt is 1 for this kernel\n"
                   "  if (rl >= A.num_rows) return;\n";
        }
        out << "  const char *const mm_xy0 = XY;\n"
               "  const float *const mm_xt = S.xtabs + col;      // this column in the table of grid column 0\n"
               "  const float *const mm_yt = S.ytabs + rl;       // this row in the table of grid row 0\n"
               "  const int mm_xend = S.gx * A.region_width, mm_yend = S.gy * A.num_rows;\n"
               "  long long mm_slot = (long long)fi * S.samples;\n"
               "  int mm_xo = 0, mm_yo = 0;                      // (wave-uniform) a * region_width, b * num_rows\n"
               "  mm_tup<4> mm_acc;\n"
               "  mm_acc.v[0] = mm_acc.v[1] = mm_acc.v[2] = mm_acc.v[3] = 0.0f;\n"
               "#pragma unroll 1\n"
               "  for (int mm_s = 0; mm_s < S.total; ++mm_s) {\n"
               "    { const mm_clip_frame mm_cf = C.frames[mm_slot]; A.t = mm_cf.t; A.frame = mm_cf.frame; }\n"
               "    const char *__restrict__ XY = mm_xy0 + mm_slot * C.xy_stride;\n"
               "    const float x = mm_xt[mm_xo];   // CALC_VIRTUAL_X(col + region_x, ..., offset a), by the prologue\n"
               "    const float y = mm_yt[mm_yo];   // CALC_VIRTUAL_Y(first_row + rl, ..., offset b)\n"
               "    MM_INTERNALS\n"
               "    unsigned mm_rand_ctr = 0;      // RAND call number within this pixel: every sub-sample is a render of its own\n"
               "    (void)XY; (void)x; (void)y; (void)mm_rand_ctr;\n";
        transfer_loads(nullptr, "    ");
        decls(pix_defs, "    ");
        stmts(code.body, PIXEL, "    ");
        out << "    mm_tup<4> rt;\n";
        for (int i = 0; i < 4; ++i) out << "    rt.v[" << i << "] = " << prim(Primary::V(code.result[i]), PIXEL) << ";\n";
        out << "    if (mm_s == 0) mm_acc = rt;\n"
               "    else\n"
               "      for (int mm_c = 0; mm_c < 4; ++mm_c) mm_acc.v[mm_c] = mm_acc.v[mm_c] + rt.v[mm_c];\n"
               "    mm_xo += A.region_width;\n"
               "    if (mm_xo == mm_xend) {\n"
               "      mm_xo = 0;\n"
               "      mm_yo += A.num_rows;\n"
               "      if (mm_yo == mm_yend) { mm_yo = 0; ++mm_slot; }\n"
               "    }\n"
               "  }\n"
               "  mm_tup<4> mm_m;\n"
               "  for (int mm_c = 0; mm_c < 4; ++mm_c) mm_m.v[mm_c] = mm_acc.v[mm_c] * S.inv_k;\n"
               "  mm_store_pixel(A, rl, col, mm_m);\n}\n";
    }

    // loop shape: A.ppt rows per work-item, MM_UNROLL of them per step
    void emit_pixel_loops() {
        // descriptors of frame-constant images, loaded (scalar) once before the pixel loop
        for (Value *v : transfer_order)
            if (v->var->type == Ty::Image) {
                out << "  const mm_image_desc " << vname(v) << "_desc = mm_load_desc(A, " << vname(v) << ");\n";
                preloaded_desc.insert(v);
            }
        // Hot variant: when every fetch through a preloaded descriptor reads a bound drawable
        // at a valid, frame-constant frame number (true for every ordinary render), those
        // conditions -- all wave-uniform -- are tested once here instead of inside each fetch,
        // which leaves the unrolled pixel bodies free of branches.  The generic loop follows it and
        // takes over from the same mm_p: for everything when the hot conditions do not hold, and for a
        // work-item that met an invalid coordinate (mm_bad), whose garbage the reference converts in a
        // way only the generic fetch imitates.
        std::vector<std::string> hot_views, hot_conds;
        find_hot_fetches(code.body, hot_views, hot_conds);
        out << "  int mm_p = 0;\n";
        if (ks.unroll > 1 && !hot_conds.empty()) {
            for (const std::string &v : hot_views) out << "  " << v << "\n";
            out << "  bool mm_hot = true;\n";
            for (const std::string &c : hot_conds) out << "  mm_hot = mm_hot && " << c << ";\n";
            out << "  if (mm_hot) {\n";
            hot_mode = true;
            fetched_result = find_fetched_result();
            emit_loop("    ", true);
            fetched_result = nullptr;
            hot_mode = false;
            out << "  }\n";
        } else {
            hot_sites.clear();
            hot_frame_sites.clear();
            site_view.clear();
        }
        emit_loop("  ", false);
        out << "}\n";
    }

    // The pixel loop.  MM_UNROLL pixels are evaluated back to back before any of them is stored: with the
    // branch-free fetch their image loads are independent and overlap (one load per wave in
    // flight cannot cover HBM latency); rows past the end are computed on the last row and
    // simply not stored.  A.ppt is a multiple of MM_UNROLL (runtime.cpp).
    void emit_loop(const std::string &I, bool hot) {
        if (pair) { pair->emit_pixel_loop(I); return; }
        const bool fetched = hot && fetched_result;
        // The row coordinates of an iteration are loaded during the one before it (those of the first before the
        // loop): a work-item's iterations are a serial chain, and the table load in front of each would add one
        // memory round trip per iteration to it.  (Rows past the end read the last row's entry.)
        out << I << "float mm_y[MM_UNROLL];\n"
            << "#pragma unroll\n" << I << "for (int mm_u = 0; mm_u < MM_UNROLL; ++mm_u) {\n"
            << I << "  const int rl_raw = row0 + (mm_p + mm_u) * MM_TILE_H;\n"
            << I << "  mm_y[mm_u] = A.ytab[rl_raw < A.num_rows ? rl_raw : A.num_rows - 1];\n"
            << I << "}\n";
        out << "#pragma unroll 1\n" << I << "for (; mm_p < A.ppt; mm_p += MM_UNROLL) {\n"
            << I << (fetched ? "  mm_bilinear mm_rs[MM_UNROLL];\n" : "  mm_tup<4> mm_rt[MM_UNROLL];\n")
            << I << "  float mm_yn[MM_UNROLL];\n"
            << I << "  bool mm_bad = false;   // a hot fetch met a NaN / inf / > 2^31 px coordinate\n"
            << "#pragma unroll\n" << I << "  for (int mm_u = 0; mm_u < MM_UNROLL; ++mm_u) {\n"
            << I << "    const int rl_raw = row0 + (mm_p + MM_UNROLL + mm_u) * MM_TILE_H;\n"
            << I << "    mm_yn[mm_u] = A.ytab[rl_raw < A.num_rows ? rl_raw : A.num_rows - 1];\n"
            << I << "  }\n"
            << "#pragma unroll\n" << I << "  for (int mm_u = 0; mm_u < MM_UNROLL; ++mm_u) {\n"
            << I << "    const float y = mm_y[mm_u];    // CALC_VIRTUAL_Y(first_row + rl, ...), once per row by the prologue\n"
            << I << "    const int rl_u = row0 + (mm_p + mm_u) * MM_TILE_H;\n"
            << I << "    const int rl = rl_u < A.num_rows ? rl_u : A.num_rows - 1;\n"
            << I << "    unsigned mm_rand_ctr = 0;      // RAND call number within this pixel\n"
            << I << "    (void)y; (void)rl; (void)mm_rand_ctr;\n";
        if (!dual_base_off.empty())
            out << I << "    int mm_dyn_ctr = 0;            // in-loop native calls made so far by this pixel's copy of a loop of both slices\n";
        row_loads(I + "    ", "rl");
        decls(pix_defs, (I + "    ").c_str());
        stmts(code.body, PIXEL, (I + "    ").c_str());
        for (int i = 0; i < 4 && !fetched; ++i)
            out << I << "    mm_rt[mm_u].v[" << i << "] = " << prim(Primary::V(code.result[i]), PIXEL) << ";\n";
        out << I << "  }\n";
        if (hot)
            out << I << "  if (mm_bad) break;     // these pixels (and this work-item's remaining ones) take the generic loop below\n";
        out << "#pragma unroll\n" << I << "  for (int mm_u = 0; mm_u < MM_UNROLL; ++mm_u) {\n"
            << I << "    // a row past the end was evaluated as the last row: storing it there again writes the\n"
            << I << "    // same bytes, and keeps the pixel bodies free of a store guard the compiler would\n"
            << I << "    // otherwise sink them (and their loads) into\n"
            << I << "    const int rl_raw = row0 + (mm_p + mm_u) * MM_TILE_H;\n"
            << I << (fetched ? "    mm_store_fetched_pixel(A, rl_raw < A.num_rows ? rl_raw : A.num_rows - 1, col, mm_rs[mm_u]);\n"
                             : "    mm_store_pixel(A, rl_raw < A.num_rows ? rl_raw : A.num_rows - 1, col, mm_rt[mm_u]);\n")
            << I << "  }\n"
            << "#pragma unroll\n" << I << "  for (int mm_u = 0; mm_u < MM_UNROLL; ++mm_u) mm_y[mm_u] = mm_yn[mm_u];\n"
            << I << "}\n";
    }
};

}  // namespace
}  // namespace hipgen

using namespace hipgen;

// What the clip kernels have besides mm_args: the batch's {t, frame} table and the distances between the frames' outputs,
// frame-constant slots and row tables (0 where all frames share one: KernelSource::prologue_uses_time false).  The entry
// block makes the by-value mm_args the frame's own -- fi is wave-uniform, so the table entry is a scalar load ahead of
// every store -- and the unchanged body follows.
const char *clip_prelude() {
    return "struct mm_clip_frame { float t; int frame; };\n"
           "struct mm_clip { const mm_clip_frame *frames; long long frame_stride; int xy_stride; int rowtab_stride; int nwg; int pad; };\n"
           "#define MM_CLIP_ENTRY \\\n"
           "  const int fi = blockIdx.y; \\\n"
           "  { const mm_clip_frame mm_cf = C.frames[fi]; A.t = mm_cf.t; A.frame = mm_cf.frame; } \\\n"
           "  A.out = (char *)A.out + (long long)fi * C.frame_stride; \\\n"
           "  XY += (long long)fi * C.xy_stride; \\\n"
           "  if (A.rowtab) A.rowtab += (long long)fi * C.rowtab_stride;\n";
}

// The same for a filter that calls native filters: every frame of a batch has an image table of its own (its native
// results), images_stride entries behind the previous frame's (0 while all frames read one table: the prologue).  A text
// of its own, so that the clip text of every other filter stays what it was.
const char *clip_prelude_natives() {
    return "struct mm_clip_frame { float t; int frame; };\n"
           "struct mm_clip { const mm_clip_frame *frames; long long frame_stride; int xy_stride; int rowtab_stride; int nwg; int images_stride; };\n"
           "#define MM_CLIP_ENTRY \\\n"
           "  const int fi = blockIdx.y; \\\n"
           "  { const mm_clip_frame mm_cf = C.frames[fi]; A.t = mm_cf.t; A.frame = mm_cf.frame; } \\\n"
           "  A.out = (char *)A.out + (long long)fi * C.frame_stride; \\\n"
           "  XY += (long long)fi * C.xy_stride; \\\n"
           "  if (A.rowtab) A.rowtab += (long long)fi * C.rowtab_stride; \\\n"
           "  A.images += (long long)fi * C.images_stride;\n";
}

// What mm_pixels_shutter has besides mm_args and mm_clip: the sub-samples of an output pixel and (float)(1.0 / samples).
const char *shutter_prelude() { return "struct mm_shutter { int samples; float inv_k; };\n"; }

// What the sampled variant's kernels have besides mm_args and mm_clip: the grid's offsets (gx along x from offs[0], gy
// along y from offs[MM_SAMPLE_GRID_MAX], in device memory: a by-value array indexed by a loop counter would be copied
// to scratch), the per-offset coordinate tables (gx * region_width and gy * num_rows floats), the shutter's sub-samples,
// total = samples * gx * gy and (float)(1.0 / total).
const char *sampled_prelude() {
    return "#define MM_SAMPLE_GRID_MAX 8\n"
           "struct mm_sampled { const float *offs; float *xtabs; float *ytabs; int samples; int gx; int gy; int total; float inv_k; int pad; };\n";
}

// What mm_pixels_refine has besides those: every frame's list of the pixels to refine (col | rl << 16, list_stride entries
// per frame) and the lists' lengths, as the mask kernel (k_aa_contrast_clip, clip_combine.hip) left them.
const char *refine_prelude() {
    return "struct mm_refine { const unsigned *list; const unsigned *counts; long long list_stride; };\n";
}

void clip_kernel_source(const KernelSource &ks, std::string *source, std::string *key) {
    source->clear();
    size_t at = 0;
    for (const KernelSource::Splice &sp : ks.clip_splices) {
        source->append(ks.source, at, sp.begin - at);
        source->append(sp.text);
        at = sp.end;
    }
    source->append(ks.source, at, std::string::npos);
    *key = text_key(*source);      // like the single-frame text's key
}

bool pair_peel_enabled() { return Knobs().pair_peel.value_or(0) != 0; }

KernelSource generate_hip(FilterCode &code, const KernelOptions &opt, FilterCode *functions_of) {
    const Knobs knobs;      // this compile's reading of the environment
    Generator g(code, opt, knobs);
    g.fn_root = functions_of;
    g.run();
    return std::move(g.ks);
}

}  // namespace mm
