// Self-test of the reference-ABI tier.  The reference itself cannot be built in this
// environment (needs clisp/bison/glib/GIMP headers), so the importer is exercised by
// exporting our own IR into the reference's structure layouts (mathmap_abi.h), then
// driving gen_and_load_hip_code() and the returned mathfuncs exactly as
// mathmap_common.c does (init_invocation :714-734, invocation_new_frame :797-816,
// invocation_init_slice :848-865, calc_lines :837-846).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>

#include "../../include/mathmap_hip_backend.h"
#include "../../include/mmhip.h"
#include "clip_kernels.h"
#include "front.h"
#include "mm_clip_filter.h"
#include "mm_sample_grid.h"
#include "runtime_internal.h"

namespace mm { void load_ir_json(Module &mod, FilterCode &code, const char *json); }   // ir_json.cpp

using namespace mm;

namespace {

struct Exporter {
    std::deque<mmabi_statement_t> stmts;
    std::deque<mmabi_rhs_t> rhss;
    std::deque<mmabi_value_t> values;
    std::deque<mmabi_compvar_t> compvars;
    std::deque<mmabi_temporary_t> temps;
    std::deque<mmabi_variable_t> variables;
    std::deque<mmabi_operation_t> ops;
    std::deque<mmabi_internal_t> internals;
    std::deque<mmabi_filter_t> filters;
    std::deque<mmabi_userval_info_t> uvinfos;
    std::deque<mmabi_option_t> options;
    std::deque<mmabi_top_level_decl_t> decls;
    std::deque<std::vector<mmabi_primary_t>> primary_arrays;
    std::deque<std::string> strings;
    std::map<const CompVar *, mmabi_compvar_t *> cv;
    std::map<const Value *, mmabi_value_t *> vv;
    std::map<const OpInfo *, mmabi_operation_t *> opmap;
    std::map<std::string, mmabi_internal_t *> intmap;
    std::map<const Filter *, mmabi_filter_t *> fmap;

    char *str(const std::string &s) {
        strings.push_back(s);
        return const_cast<char *>(strings.back().c_str());
    }

    mmabi_compvar_t *compvar(const CompVar *c) {
        auto it = cv.find(c);
        if (it != cv.end()) return it->second;
        compvars.emplace_back();
        mmabi_compvar_t *r = &compvars.back();
        memset(r, 0, sizeof *r);
        r->index = c->id;
        r->type = (int)c->type;
        r->n = c->elem;
        if (c->is_temp) {
            temps.emplace_back();
            temps.back().number = c->id;
            r->temp = &temps.back();
        } else {
            variables.emplace_back();
            memset(&variables.back(), 0, sizeof(mmabi_variable_t));
            variables.back().name = str(c->name);
            r->var = &variables.back();
        }
        cv[c] = r;
        return r;
    }

    mmabi_value_t *value(const Value *v) {
        auto it = vv.find(v);
        if (it != vv.end()) return it->second;
        values.emplace_back();
        mmabi_value_t *r = &values.back();
        memset(r, 0, sizeof *r);
        r->compvar = compvar(v->var);
        r->index = v->index;
        r->global_index = v->gid;
        vv[v] = r;
        return r;
    }

    mmabi_primary_t primary(const Primary &p) {
        mmabi_primary_t r;
        memset(&r, 0, sizeof r);
        switch (p.kind) {
            case Primary::Val: r.kind = MMABI_PRIMARY_VALUE; r.v.value = value(p.value); break;
            case Primary::IntConst: r.kind = MMABI_PRIMARY_CONST; r.const_type = MMABI_TYPE_INT; r.v.constant.int_value = p.i; break;
            case Primary::FloatConst: r.kind = MMABI_PRIMARY_CONST; r.const_type = MMABI_TYPE_FLOAT; r.v.constant.float_value = p.f; break;
            default: r.kind = MMABI_PRIMARY_CONST; r.const_type = MMABI_TYPE_INT; break;
        }
        return r;
    }

    mmabi_filter_t *filter(const Filter *f) {
        auto it = fmap.find(f);
        if (it != fmap.end()) return it->second;
        filters.emplace_back();
        mmabi_filter_t *r = &filters.back();
        memset(r, 0, sizeof *r);
        r->name = str(f->name);
        r->num_uservals = (int)f->uservals.size();
        mmabi_userval_info_t *prev = nullptr;
        for (const UservalInfo &u : f->uservals) {
            uvinfos.emplace_back();
            mmabi_userval_info_t *ui = &uvinfos.back();
            memset(ui, 0, sizeof *ui);
            ui->name = str(u.name);
            ui->index = u.index;
            switch (u.kind) {
                case UvKind::Int: ui->type = MMABI_USERVAL_INT_CONST; ui->v.int_const.min = u.imin; ui->v.int_const.max = u.imax; ui->v.int_const.default_value = u.idef; break;
                case UvKind::Float: ui->type = MMABI_USERVAL_FLOAT_CONST; ui->v.float_const.min = u.fmin; ui->v.float_const.max = u.fmax; ui->v.float_const.default_value = u.fdef; break;
                case UvKind::Bool: ui->type = MMABI_USERVAL_BOOL_CONST; ui->v.bool_const.default_value = u.bdef; break;
                case UvKind::Color: ui->type = MMABI_USERVAL_COLOR; break;
                case UvKind::Curve: ui->type = MMABI_USERVAL_CURVE; break;
                case UvKind::Gradient: ui->type = MMABI_USERVAL_GRADIENT; break;
                case UvKind::Image: ui->type = MMABI_USERVAL_IMAGE; ui->v.image.flags = u.image_flags; break;
            }
            if (prev) prev->next = ui; else r->userval_infos = ui;
            prev = ui;
        }
        if (f->kind == Filter::Native) {
            r->kind = MMABI_FILTER_NATIVE;
            r->v.native.func_name = str(f->native_func);
            r->v.native.is_pure = 1;
        } else {
            r->kind = MMABI_FILTER_MATHMAP;
            decls.emplace_back();
            mmabi_top_level_decl_t *d = &decls.back();
            memset(d, 0, sizeof *d);
            d->name = r->name;
            auto add_opt = [&](const char *n) {
                options.emplace_back();
                options.back().name = str(n);
                options.back().suboptions = nullptr;
                options.back().next = d->v.filter.options;
                d->v.filter.options = &options.back();
            };
            if (!(f->flags & IMAGE_FLAG_UNIT)) add_opt("pixel");
            else if (!(f->flags & IMAGE_FLAG_SQUARE)) add_opt("stretched");
            r->v.mathmap.decl = d;
        }
        fmap[f] = r;
        return r;
    }

    mmabi_rhs_t *rhs(const Rhs &s) {
        rhss.emplace_back();
        mmabi_rhs_t *r = &rhss.back();
        memset(r, 0, sizeof *r);
        switch (s.kind) {
            case Rhs::Prim: r->kind = MMABI_RHS_PRIMARY; r->v.primary = primary(s.prim); break;
            case Rhs::Internal: {
                r->kind = MMABI_RHS_INTERNAL;
                auto it = intmap.find(s.internal);
                if (it == intmap.end()) {
                    internals.emplace_back();
                    memset(&internals.back(), 0, sizeof(mmabi_internal_t));
                    strncpy(internals.back().name, s.internal.c_str(), 63);
                    it = intmap.emplace(s.internal, &internals.back()).first;
                }
                r->v.internal = it->second;
                break;
            }
            case Rhs::Op: {
                r->kind = MMABI_RHS_OP;
                auto it = opmap.find(s.op);
                if (it == opmap.end()) {
                    ops.emplace_back();
                    mmabi_operation_t *o = &ops.back();
                    memset(o, 0, sizeof *o);
                    o->index = s.op->index;
                    o->name = str(s.op->cname);
                    o->num_args = s.op->nargs;
                    it = opmap.emplace(s.op, o).first;
                }
                r->v.op.op = it->second;
                for (size_t i = 0; i < s.args.size(); ++i) r->v.op.args[i] = primary(s.args[i]);
                break;
            }
            case Rhs::Closure: {
                r->kind = MMABI_RHS_CLOSURE;
                r->v.closure.filter = filter(s.filter);
                primary_arrays.emplace_back();
                for (const Primary &p : s.args) primary_arrays.back().push_back(primary(p));
                r->v.closure.args = primary_arrays.back().data();
                break;
            }
            case Rhs::Tuple:
            case Rhs::TreeVector: {
                r->kind = s.kind == Rhs::Tuple ? MMABI_RHS_TUPLE : MMABI_RHS_TREE_VECTOR;
                r->v.tuple.length = (int)s.args.size();
                primary_arrays.emplace_back();
                for (const Primary &p : s.args) primary_arrays.back().push_back(primary(p));
                r->v.tuple.args = primary_arrays.back().data();
                break;
            }
            case Rhs::None: break;
            case Rhs::FilterCall: {
                r->kind = MMABI_RHS_FILTER;
                r->v.filter.filter = filter(s.filter);
                primary_arrays.emplace_back();
                for (const Primary &p : s.args) primary_arrays.back().push_back(primary(p));
                r->v.filter.args = primary_arrays.back().data();
                break;
            }
        }
        return r;
    }

    mmabi_statement_t *new_stmt(int kind) {
        stmts.emplace_back();
        mmabi_statement_t *s = &stmts.back();
        memset(s, 0, sizeof *s);
        s->kind = kind;
        return s;
    }

    mmabi_statement_t *phis(const Block &b) {
        mmabi_statement_t *first = nullptr, **tail = &first;
        for (const Stmt *p : b) {
            if (p->kind != Stmt::Phi) continue;
            mmabi_statement_t *s = new_stmt(MMABI_STMT_PHI_ASSIGN);
            s->v.assign.lhs = value(p->lhs);
            s->v.assign.rhs = rhs(p->rhs);
            s->v.assign.rhs2 = rhs(p->rhs2);
            *tail = s;
            tail = &s->next;
        }
        if (!first) first = new_stmt(MMABI_STMT_NIL);   // the reference terminates empty lists with a NIL statement
        return first;
    }

    mmabi_statement_t *block(const Block &b) {
        mmabi_statement_t *first = nullptr, **tail = &first;
        for (const Stmt *st : b) {
            mmabi_statement_t *s = nullptr;
            switch (st->kind) {
                case Stmt::Assign:
                    s = new_stmt(MMABI_STMT_ASSIGN);
                    s->v.assign.lhs = value(st->lhs);
                    s->v.assign.rhs = rhs(st->rhs);
                    break;
                case Stmt::If:
                    s = new_stmt(MMABI_STMT_IF_COND);
                    s->v.if_cond.condition = rhs(st->cond);
                    s->v.if_cond.consequent = block(st->then_);
                    s->v.if_cond.alternative = block(st->else_);
                    s->v.if_cond.exit = phis(st->phis);
                    break;
                case Stmt::While:
                    s = new_stmt(MMABI_STMT_WHILE_LOOP);
                    s->v.while_loop.entry = phis(st->phis);
                    s->v.while_loop.invariant = rhs(st->cond);
                    s->v.while_loop.body = block(st->body);
                    break;
                default: continue;
            }
            *tail = s;
            tail = &s->next;
        }
        if (!first) first = new_stmt(MMABI_STMT_NIL);
        return first;
    }
};

const uint8_t *g_img = nullptr;
int g_iw = 0, g_ih = 0, g_ic = 3;

mmabi_color_t selftest_get_pixel(mmabi_invocation_t *inv, mmabi_input_drawable_t *d, int frame, int x, int y) {
    // mathmap.c:1195-1209 + mathmap_cmdline.c:131-184
    if (x < 0 || x >= d->image.pixel_width) return inv->edge_color_x;
    if (y < 0 || y >= d->image.pixel_height) return inv->edge_color_y;
    (void)frame;
    const uint8_t *p = g_img + (size_t)g_ic * ((size_t)g_iw * y + x);
    return ((mmabi_color_t)p[0] << 24) | ((mmabi_color_t)p[1] << 16) | ((mmabi_color_t)p[2] << 8) | (g_ic == 4 ? p[3] : 255u);
}

thread_local std::string g_selftest_err;

}  // namespace

extern "C" {

const char *mmhip_selftest_error(void) { return g_selftest_err.c_str(); }

// the host's drawable_get_pixel_inc (mathmap.h:314; mathmap.c:1320-1327): the stride of the image sources, > 1 while
// the GIMP dialog previews.  The backend finds it by name, like a compiled module would.
static int g_pixel_inc = 1;
void drawable_get_pixel_inc(void *, void *, int *inc_x, int *inc_y) { *inc_x = *inc_y = g_pixel_inc; }
void mmhip_selftest_set_pixel_inc(int inc) { g_pixel_inc = inc; }

// the host's error buffer: the backend reports through it like the reference's backends do (exprtree.c:40, cc.c:653-693)
char error_string[1024];

// Compiles `source` with our front-end, exports the (un-optimised) IR into reference-layout
// structures, pushes it through gen_and_load_hip_code and renders a w x h frame through the
// returned mathfuncs into `out_rgba` (w*h*4 bytes).  Returns 0 on success.
int mmhip_selftest_abi_roundtrip(const char *source, int intersample, const uint8_t *image, int iw, int ih, int ichannels,
                                 int w, int h, float t, int num_bands, uint8_t *out_rgba) {
    try {
        // `source`: .mm text, or -- first character '{' -- an IR dump (mmhip_filter_ir_json_raw's form): the
        // reference's own filters are kept as IR fixtures only (tests/filters.py)
        Module m;
        std::unique_ptr<FilterCode> code;
        const char *first = source;
        while (*first == ' ' || *first == '\n' || *first == '\t' || *first == '\r') ++first;
        const bool from_ir = *first == '{';
        if (from_ir) {
            code.reset(new FilterCode());
            load_ir_json(m, *code, source);
        } else {
            parse_module(m, source);
            code = lower_filter(m, m.main);
        }

        Exporter ex;
        // filter list in module order (native filters first, like register_native_filters
        // runs before parsing, mathmap_common.c:411-421)
        std::vector<mmabi_filter_t *> flist;
        for (auto &f : m.filters) flist.push_back(ex.filter(f.get()));
        for (size_t i = 0; i + 1 < flist.size(); ++i) flist[i]->next = flist[i + 1];

        // body + `tuple = (r,g,b,a); dummy = OUTPUT_TUPLE(tuple)` (compiler.c:4692-4697), for the main filter and
        // for every filter it calls at run time (compiler_compile_filters hands the backend one code per filter)
        auto export_code = [&](FilterCode &c, mmabi_filter_code_t &out) {
            CompVar *tuple = c.new_var(Ty::Tuple);
            tuple->tuple_len = 4;
            Stmt *ta = c.new_stmt(Stmt::Assign);
            ta->lhs = c.new_value(tuple);
            ta->rhs.kind = Rhs::Tuple;
            for (int i = 0; i < 4; ++i) ta->rhs.args.push_back(Primary::V(c.result[i]));
            c.body.push_back(ta);
            CompVar *dummy = c.new_var(Ty::Int);
            Stmt *oa = c.new_stmt(Stmt::Assign);
            oa->lhs = c.new_value(dummy);
            oa->rhs = Rhs::O(op_by_cname("OUTPUT_TUPLE", 1), {Primary::V(ta->lhs)});
            c.body.push_back(oa);
            out.first_stmt = ex.block(c.body);
        };
        mmabi_filter_code_t fc;
        fc.filter = ex.filter(m.main);
        export_code(*code, fc);
        std::deque<mmabi_filter_code_t> fn_codes;
        std::vector<const Filter *> have;
        for (auto &fn : code->functions) {
            fn_codes.emplace_back();
            fn_codes.back().filter = ex.filter(fn->filter);
            export_code(*fn, fn_codes.back());
            have.push_back(fn->filter);
        }
        // the reference hands the backend a code for *every* filter of the module (compiler_compile_filters); the ones a
        // backend can need besides the called ones are the filters whose closures are made in the main code (a closure
        // image given to a native filter is rendered by its own filter's code)
        std::vector<std::unique_ptr<FilterCode>> closure_codes;
        std::function<void(const Block &)> find_closures = [&](const Block &b) {
            for (const Stmt *st : b) {
                if (st->kind == Stmt::Assign && st->rhs.kind == Rhs::Closure && st->rhs.filter->kind == Filter::MathMap &&
                    st->rhs.filter != m.main && std::find(have.begin(), have.end(), st->rhs.filter) == have.end()) {
                    have.push_back(st->rhs.filter);
                    // an IR dump carries no bodies of the filters whose closures it applies inline: no code to hand over (the
                    // backend asks for one only when the closure image reaches a native filter, and reports that itself)
                    if (from_ir) continue;
                    closure_codes.push_back(lower_function(m, const_cast<Filter *>(st->rhs.filter)));
                    fn_codes.emplace_back();
                    fn_codes.back().filter = ex.filter(st->rhs.filter);
                    export_code(*closure_codes.back(), fn_codes.back());
                }
                if (st->kind == Stmt::If) { find_closures(st->then_); find_closures(st->else_); }
                if (st->kind == Stmt::While) find_closures(st->body);
            }
        };
        find_closures(code->body);

        std::vector<mmabi_filter_code_t *> codes(flist.size(), nullptr);
        for (size_t i = 0; i < flist.size(); ++i) {
            if (flist[i] == fc.filter) codes[i] = &fc;
            for (mmabi_filter_code_t &c : fn_codes)
                if (flist[i] == c.filter && !(c.filter == fc.filter)) codes[i] = &c;
        }

        mmabi_mathmap_t mathmap;
        memset(&mathmap, 0, sizeof mathmap);
        mathmap.filters = flist.empty() ? nullptr : flist[0];
        mathmap.main_filter = fc.filter;

        g_img = image; g_iw = iw; g_ih = ih; g_ic = ichannels;
        mathmap_hip_set_get_pixel(selftest_get_pixel);
        mathmap.initfunc = gen_and_load_hip_code(&mathmap, &mathmap.module_info, nullptr, nullptr, codes.data());
        if (!mathmap.initfunc) { g_selftest_err = std::string("gen_and_load_hip_code failed: ") + error_string + mmhip_last_error(); return -1; }

        // invoke_mathmap defaults (mathmap_common.c:746-795)
        mmabi_invocation_t inv;
        memset(&inv, 0, sizeof inv);
        inv.mathmap = &mathmap;
        inv.antialiasing = intersample;
        inv.output_bpp = 4;
        inv.edge_behaviour_x = inv.edge_behaviour_y = 1;
        inv.img_width = inv.render_width = w;
        inv.img_height = inv.render_height = h;
        inv.image_R = (float)sqrt(2.0);
        inv.row_stride = w * 4;
        std::vector<unsigned char> rows_finished(h, 0);
        inv.rows_finished = rows_finished.data();
        inv.mathfuncs = mathmap.initfunc(&inv);

        // closure image with the user values (closure_image_alloc, drawable.c:230-249)
        size_t nuv = m.main->uservals.size();
        std::vector<char> closure_mem(sizeof(mmabi_image_t) + (nuv + 1) * sizeof(mmabi_userval_t), 0);
        mmabi_image_t *closure = (mmabi_image_t *)closure_mem.data();
        closure->type = MMABI_IMAGE_CLOSURE;
        closure->pixel_width = w;
        closure->pixel_height = h;
        closure->v.closure.funcs = &inv.mathfuncs;
        closure->v.closure.num_args = (int)nuv;
        mmabi_input_drawable_t drawable;
        memset(&drawable, 0, sizeof drawable);
        drawable.used = 1;
        drawable.kind = 2;
        drawable.image.type = MMABI_IMAGE_DRAWABLE;
        drawable.image.pixel_width = iw;
        drawable.image.pixel_height = ih;
        drawable.image.v.drawable = &drawable;
        drawable.scale_x = (float)((iw - 1) / 2.0);
        drawable.scale_y = (float)((ih - 1) / 2.0);
        drawable.middle_x = drawable.middle_y = 1.0f;
        std::deque<std::vector<float>> curve_tabs;
        std::deque<std::vector<mmabi_color_t>> grad_tabs;
        std::deque<mmabi_curve_t> curves;
        std::deque<mmabi_gradient_t> grads;
        for (const UservalInfo &u : m.main->uservals) {
            mmabi_userval_t &a = closure->v.closure.args[u.index];
            switch (u.kind) {
                case UvKind::Int: a.v.int_const = u.idef; break;
                case UvKind::Float: a.v.float_const = u.fdef; break;
                case UvKind::Bool: a.v.bool_const = u.bdef; break;
                case UvKind::Color: a.v.color.value = 0x000000ffu; break;
                case UvKind::Image: a.v.image = image ? &drawable.image : nullptr; break;
                // the deterministic tables of mathmap_amd/workloads.py test_curve / test_gradient
                case UvKind::Curve:
                    curve_tabs.emplace_back(1024);
                    for (int i = 0; i < 1024; ++i) curve_tabs.back()[i] = ((float)i * (float)i) / (float)(1023.0 * 1023.0);
                    curves.emplace_back();
                    memset(&curves.back(), 0, sizeof(mmabi_curve_t));
                    curves.back().values = curve_tabs.back().data();
                    a.v.curve = &curves.back();
                    break;
                case UvKind::Gradient:
                    grad_tabs.emplace_back(1024);
                    for (unsigned i = 0; i < 1024; ++i)
                        grad_tabs.back()[i] = ((i >> 2) << 24) | (((1023 - i) >> 2) << 16) | (0x40u << 8) | 0xFFu;
                    grads.emplace_back();
                    grads.back().values = grad_tabs.back().data();
                    a.v.gradient = &grads.back();
                    break;
                default: break;
            }
        }
        inv.uservals = closure->v.closure.args;

        mmabi_frame_t frame;
        memset(&frame, 0, sizeof frame);
        frame.invocation = &inv;
        frame.frame_render_width = w;
        frame.frame_render_height = h;
        frame.current_frame = 0;
        // MMHIP_SELFTEST_WARM_FRAMES=n: render n earlier frames (t - n/16 ... t - 1/16) first, like an
        // animation; from its 2nd frame on the backend runs the user-value-specialised variant
        int warm = 0;
        if (const char *e = getenv("MMHIP_SELFTEST_WARM_FRAMES")) warm = atoi(e);
        if (num_bands < 1) num_bands = 1;
        for (int wf = warm; wf >= 0; --wf) {
        std::fill(rows_finished.begin(), rows_finished.end(), 0);
        frame.current_t = t - (float)wf / 16.0f;
        inv.mathfuncs.init_frame(&frame, closure);
        // call_invocation_parallel (mathmap_common.c:972-1006): contiguous row bands
        for (int b = 0; b < num_bands; ++b) {
            int lo = h * b / num_bands, hi = h * (b + 1) / num_bands;
            mmabi_slice_t slice;
            memset(&slice, 0, sizeof slice);
            slice.frame = &frame;
            slice.region_x = 0;
            slice.region_y = lo;
            slice.region_width = w;
            slice.region_height = hi - lo;
            inv.mathfuncs.init_slice(&slice, closure);
            inv.mathfuncs.calc_lines(&slice, closure, lo, hi, out_rgba + (size_t)lo * inv.row_stride, 0);
        }
        }
        int finished = 0;
        for (int r = 0; r < h; ++r) finished += rows_finished[r];
        unload_hip_code(mathmap.module_info);
        mathmap_hip_set_get_pixel(nullptr);
        // the template indexes rows_finished with the slice-relative row (new_template.c.in:307-308),
        // so with several bands only the first max-band-height entries are set
        int expect = 0;
        for (int b = 0; b < num_bands; ++b) expect = std::max(expect, h * (b + 1) / num_bands - h * b / num_bands);
        if (finished != expect) {
            g_selftest_err = "rows_finished bookkeeping differs from the template's";
            if (error_string[0]) g_selftest_err += std::string(" (the backend reported: ") + error_string + ")";
            return -2;
        }
        return 0;
    } catch (const std::exception &e) {
        g_selftest_err = e.what();
        return -3;
    }
}

// gaussian_blur(in, hdev, vdev) of an RGB8 host image through the tolerance chain (mmhip_options.gauss_mode), with the
// float map written as well -- the product never writes it on that chain (nothing reads it) -- into `map`
// (float[h][w][4]), so that a test can bound its float error directly.  0 on success.
int mmhip_selftest_gauss_tolerance_map(const uint8_t *rgb, int w, int h, float hdev, float vdev, float *map) {
    static const char *src = "stretched filter gauss_direct (stretched image in, float hdev: 0-1 (0.01), float vdev: 0-1 (0.01))\n"
                             "  soft = gaussian_blur(in, hdev, vdev);\n"
                             "  soft(xy)\n"
                             "end\n";
    mmhip_options o;
    mmhip_default_options(&o);
    o.gauss_mode = MMHIP_GAUSS_TOLERANCE;
    std::unique_ptr<mmhip_filter, void (*)(mmhip_filter *)> f(mmhip_compile(src, &o), mmhip_filter_free);
    if (!f || mmhip_filter_jit(f.get(), 1) < 0) { g_selftest_err = mmhip_last_error(); return -1; }
    std::unique_ptr<mmhip_invocation, void (*)(mmhip_invocation *)> inv(mmhip_invoke(f.get(), w, h), mmhip_invocation_free);
    if (!inv) { g_selftest_err = mmhip_last_error(); return -1; }
    std::unique_ptr<void, void (*)(void *)> out(mmhip_device_alloc((size_t)w * h * 4), mmhip_device_free);
    char hv[32], vv[32];
    snprintf(hv, sizeof hv, "%.9g", hdev);
    snprintf(vv, sizeof vv, "%.9g", vdev);
    inv->ws.keep_tolerance_map = true;
    if (!out || mmhip_set_by_name(inv.get(), "hdev", hv) != 0 || mmhip_set_by_name(inv.get(), "vdev", vv) != 0 ||
        mmhip_set_image_host(inv.get(), 0, rgb, w, h, 3) != 0 ||
        mmhip_render(inv.get(), 0, 0.0f, 0, 0, w, h, 0, h, out.get(), w * 4, 4, 0, nullptr) != 0 || mmhip_sync(inv.get()) != 0) {
        g_selftest_err = out ? mmhip_last_error() : "out of device memory";
        return -1;
    }
    if (inv->tolerance_blur_launches != 1 || inv->natives.size() != 1 || !inv->natives[0].map) {
        g_selftest_err = "the render did not take the tolerance chain";
        return -2;
    }
    return mmhip_copy_to_host(map, inv->natives[0].map.get(), (size_t)w * h * 16) == 0 ? 0 : -1;
}

// {segment length, halo, number of segments} of one pass of gaussian_blur's recursive path (mm::gaussian_blur_line_plan):
// what a test needs to restate a split pass segment by segment.
void mmhip_selftest_gauss_line_plan(int n, int lines, float sigma, int tolerance, int *out) {
    mm::gaussian_blur_line_plan(n, lines, sigma, tolerance, out);
}

// The two supersampling combines on the same slices (tools/clip_ss_cost.py, tests/test_gpu_clip_supersample.py): `frames`
// frames of w x h slices of pseudo-random bytes (every frame its own copy, for either kernel), combined frame by frame by launch_supersample_combine (what
// mmhip_render_supersampled runs) and by one launch_supersample_combine_clip, alternating for `rounds` rounds with device
// events around each; ms[2 * r] receives the old kernel's milliseconds for all frames of round r, ms[2 * r + 1] the new
// one's.  Returns the number of output bytes in which the two differ (0 is what is wanted), or -1.
long mmhip_selftest_combine_ms(int w, int h, int bpp, int frames, int rounds, double *ms) {
    if (w < 1 || h < 1 || bpp < 1 || bpp > 4 || frames < 1 || frames > 65535 || rounds < 1) { g_selftest_err = "combine: bad arguments"; return -1; }
    const size_t packed = (size_t)(w + 1) * bpp, pitch = mm::supersample_clip_long_pitch(w, bpp), short_row = (size_t)w * bpp;
    const size_t long_old = packed * h, long_new = pitch * h, short_bytes = short_row * h, out_bytes = short_row * h;
    std::vector<unsigned char> host(long_old + short_bytes);
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (size_t i = 0; i < host.size(); ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        host[i] = (unsigned char)(x >> 32);
    }
    DeviceBuffer old_slices, new_longs, new_shorts, out_old, out_new;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto ok = [](hipError_t e) { if (e != hipSuccess) g_selftest_err = std::string("combine: ") + hipGetErrorString(e); return e == hipSuccess; };
    long result = -1;
    std::string err;
    mm::NativeWorkspace ws;
    do {
        if (!ok(old_slices.grow(host.size() * frames)) || !ok(new_longs.grow(long_new * frames)) || !ok(new_shorts.grow(short_bytes * frames)) ||
            !ok(out_old.grow(out_bytes * frames)) || !ok(out_new.grow(out_bytes * frames)) || !ok(hipEventCreate(&e0)) || !ok(hipEventCreate(&e1)))
            break;
        if (!ok(hipMemcpy(old_slices.get(), host.data(), host.size(), hipMemcpyHostToDevice)) || !ok(hipMemset(new_longs.get(), 0x5a, long_new * frames)))
            break;
        bool copied = true;
        for (int i = 0; i < frames && copied; ++i)
            copied = (i == 0 || ok(hipMemcpy(old_slices.get<unsigned char>() + i * host.size(), old_slices.get(), host.size(), hipMemcpyDeviceToDevice))) &&
                     ok(hipMemcpy2D(new_longs.get<unsigned char>() + i * long_new, pitch, old_slices.get(), packed, packed, h, hipMemcpyDeviceToDevice)) &&
                     ok(hipMemcpy(new_shorts.get<unsigned char>() + i * short_bytes, old_slices.get<unsigned char>() + long_old, short_bytes, hipMemcpyDeviceToDevice));
        if (!copied) break;
        bool ran = true;
        for (int r = -1; r < rounds && ran; ++r) {          // round -1 warms up
            float t_old = 0, t_new = 0;
            ran = ok(hipEventRecord(e0, nullptr));
            for (int i = 0; i < frames; ++i)
                mm::launch_supersample_combine(old_slices.get<unsigned char>() + i * host.size(), old_slices.get<unsigned char>() + i * host.size() + long_old,
                                               out_old.get<unsigned char>() + i * out_bytes, w, h, bpp, (int)short_row, nullptr);
            ran = ran && ok(hipEventRecord(e1, nullptr)) && ok(hipEventSynchronize(e1)) && ok(hipEventElapsedTime(&t_old, e0, e1)) && ok(hipEventRecord(e0, nullptr));
            if (ran && mm::launch_supersample_combine_clip(new_longs.get<unsigned char>(), new_shorts.get<unsigned char>(), out_new.get<unsigned char>(), w, h,
                                                          bpp, (int)short_row, (int64_t)out_bytes, frames, ws, nullptr, &err) != 0) {
                g_selftest_err = err;
                ran = false;
            }
            ran = ran && ok(hipEventRecord(e1, nullptr)) && ok(hipEventSynchronize(e1)) && ok(hipEventElapsedTime(&t_new, e0, e1));
            if (r >= 0) { ms[2 * r] = t_old; ms[2 * r + 1] = t_new; }
        }
        if (!ran) break;
        std::vector<unsigned char> a(out_bytes), b(out_bytes);
        long differ = 0;
        bool read = true;
        for (int i = 0; i < frames && read; ++i) {
            read = ok(hipMemcpy(a.data(), out_old.get<unsigned char>() + i * out_bytes, out_bytes, hipMemcpyDeviceToHost)) &&
                   ok(hipMemcpy(b.data(), out_new.get<unsigned char>() + i * out_bytes, out_bytes, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < out_bytes && read; ++k) differ += a[k] != b[k];
        }
        if (read) result = differ;
    } while (false);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return result;
}

// The shutter combine alone (tests/test_gpu_clip_shutter.py, tools/clip_shutter_cost.py): launch_shutter_combine_clip on
// `frames` frames of `samples` sub-sample maps each, `maps` = float[frames][samples][rows][render_w][4] on the host (null:
// maps of 0.25, for timing at sizes no host array should have).  samples_per_pass below 1 or from `samples` up: one
// pass; else passes of that many sub-samples joined by a carry map, as mmhip_render_clip_shutter cuts them.  The output
// buffer of out_bytes bytes is filled with `sentinel` bytes first, frame i is written at out_offset + i * frame_stride,
// and the whole buffer is copied to `out` (null: not copied).  With rounds > 0 the passes run `rounds` more times with
// device events around each round: ms[r] receives round r's milliseconds.  Returns 0, or -1 (mmhip_selftest_error).
int mmhip_selftest_shutter_combine(const float *maps, int frames, int samples, int rows, int region_w, int render_w, int bpp,
                                   int floatmap, int row_stride, int64_t frame_stride, int samples_per_pass, int out_offset,
                                   unsigned char *out, int64_t out_bytes, int sentinel, int rounds, double *ms) {
    const int64_t band = floatmap ? (int64_t)rows * 16 * render_w : (int64_t)(rows - 1) * row_stride + (int64_t)region_w * bpp;
    if (frames < 1 || frames > 65535 || samples < 1 || samples > MMHIP_SHUTTER_MAX_SAMPLES || rows < 1 || region_w < 1 || render_w < region_w ||
        bpp < 1 || bpp > 4 || out_offset < 0 || row_stride < 0 || frame_stride < band ||
        out_bytes < out_offset + (int64_t)(frames - 1) * frame_stride + band || (rounds > 0 && !ms)) {
        g_selftest_err = "shutter combine: bad arguments";
        return -1;
    }
    if (samples_per_pass < 1 || samples_per_pass > samples) samples_per_pass = samples;
    const size_t map_bytes = (size_t)rows * render_w * 16, all = map_bytes * samples * frames;
    DeviceBuffer subs, carry, dst;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto ok = [](hipError_t e) { if (e != hipSuccess) g_selftest_err = std::string("shutter combine: ") + hipGetErrorString(e); return e == hipSuccess; };
    int result = -1;
    mm::NativeWorkspace ws;
    const float inv_k = (float)(1.0 / (double)samples);
    // every pass of every frame, in the order the runtime launches them
    auto run = [&]() {
        std::string err;
        for (int j0 = 0; j0 < samples; j0 += samples_per_pass) {
            const int count = std::min(samples_per_pass, samples - j0);
            const bool last = j0 + count >= samples;
            const mm::ClipSamples in{subs.get<unsigned char>() + (size_t)j0 * map_bytes, (int64_t)map_bytes, (int64_t)(map_bytes * samples), count,
                                     j0 > 0 ? carry.get() : nullptr, last ? nullptr : carry.get()};
            const mm::ClipStore to{dst.get<unsigned char>() + out_offset, row_stride, frame_stride, bpp, floatmap};
            if (mm::launch_shutter_combine_clip(in, to, region_w, rows, render_w, inv_k, frames, ws, nullptr, &err) != 0) {
                g_selftest_err = err;
                return false;
            }
        }
        return true;
    };
    do {
        if (!ok(subs.grow(all)) || !ok(dst.grow((size_t)out_bytes)) || (samples_per_pass < samples && !ok(carry.grow(map_bytes * frames)))) break;
        if (maps ? !ok(hipMemcpy(subs.get(), maps, all, hipMemcpyHostToDevice)) : !ok(hipMemsetD32((hipDeviceptr_t)subs.get(), 0x3e800000, all / 4))) break;
        if (!ok(hipMemset(dst.get(), sentinel, (size_t)out_bytes))) break;
        if (!run() || !ok(hipDeviceSynchronize())) break;
        if (out && !ok(hipMemcpy(out, dst.get(), (size_t)out_bytes, hipMemcpyDeviceToHost))) break;
        bool timed = true;
        if (rounds > 0) timed = ok(hipEventCreate(&e0)) && ok(hipEventCreate(&e1));
        for (int r = 0; r < rounds && timed; ++r) {
            float t = 0;
            timed = ok(hipEventRecord(e0, nullptr)) && run() && ok(hipEventRecord(e1, nullptr)) && ok(hipEventSynchronize(e1)) && ok(hipEventElapsedTime(&t, e0, e1));
            ms[r] = t;
        }
        if (timed) result = 0;
    } while (false);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return result;
}

// The filter combine alone (tests/test_gpu_clip_filtered.py, tools/clip_filter_cost.py): launch_filter_combine_clip over
// `frames` frames of `steps` time steps of an sx x sy grid, for the output rectangle of region_w columns from region_x by
// `rows` rows from first_row of a render_w x render_h frame.  `maps` = float[frames][steps][sy * sx][halo_rows][render_w][4]
// on the host, the haloed rectangle of mmhip_render_clip_filtered with its columns at the start of each row (null: maps
// of 0.25, for timing).  The tap blocks are built from mm_clip_filter.h as the runtime builds them.  steps_per_pass,
// the output buffer, `sentinel`, `rounds` and `ms` are mmhip_selftest_shutter_combine's.  Returns 0, or -1.
int mmhip_selftest_filter_combine(const float *maps, int frames, int steps, int sx, int sy, int kernel, float radius, int render_w,
                                  int render_h, int region_x, int first_row, int region_w, int rows, int bpp, int floatmap,
                                  int row_stride, int64_t frame_stride, int steps_per_pass, int out_offset, unsigned char *out,
                                  int64_t out_bytes, int sentinel, int rounds, double *ms) {
    const int64_t band = floatmap ? (int64_t)rows * 16 * render_w : (int64_t)(rows - 1) * row_stride + (int64_t)region_w * bpp;
    if (frames < 1 || frames > 65535 || steps < 1 || sx < 1 || sx > MM_SAMPLE_GRID_MAX || sy < 1 || sy > MM_SAMPLE_GRID_MAX ||
        steps * sx * sy > MMHIP_SHUTTER_MAX_SAMPLES || kernel < 0 || kernel >= MM_CLIP_FILTER_KERNELS || !(radius >= 0.5f && radius <= 4.0f) ||
        render_w < 1 || render_h < 1 || region_x < 0 || first_row < 0 || region_w < 1 || rows < 1 || (int64_t)region_x + region_w > render_w ||
        (int64_t)first_row + rows > render_h || bpp < 1 || bpp > 4 || out_offset < 0 || row_stride < 0 || frame_stride < band ||
        out_bytes < out_offset + (int64_t)(frames - 1) * frame_stride + band || (rounds > 0 && !ms)) {
        g_selftest_err = "filter combine: bad arguments";
        return -1;
    }
    if (steps_per_pass < 1 || steps_per_pass > steps) steps_per_pass = steps;
    const int reach = mm_clip_filter_reach((double)radius), grid = sx * sy;
    const int hx0 = std::max(0, region_x - reach), hy0 = std::max(0, first_row - reach);
    const int hw = std::min(render_w, region_x + region_w + reach) - hx0, hrows = std::min(render_h, first_row + rows + reach) - hy0;
    const size_t map_bytes = (size_t)hrows * render_w * 16, all = map_bytes * grid * steps * frames;
    // the blocks of both axes, x first
    std::vector<unsigned> tables;
    size_t y_tables = 0;
    for (int axis = 0; axis < 2; ++axis) {
        const int n = axis ? sy : sx;
        float offs[MM_SAMPLE_GRID_MAX];
        for (int a = 0; a < n; ++a) offs[a] = mm_sample_grid_offset(a, n);
        if (axis) y_tables = tables.size();
        const size_t at = tables.size();
        tables.resize(at + (size_t)(reach + 1) * (reach + 1) * mm_clip_filter_block_words(mm_clip_filter_tap_count(reach, n)));
        if (mm_clip_filter_axis_blocks(kernel, (double)radius, n, offs, axis ? render_h : render_w, tables.data() + at) != 0) {
            g_selftest_err = "filter combine: the weights do not sum to a positive finite number";
            return -1;
        }
    }
    DeviceBuffer subs, carry, dst, taps_dev;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto ok = [](hipError_t e) { if (e != hipSuccess) g_selftest_err = std::string("filter combine: ") + hipGetErrorString(e); return e == hipSuccess; };
    int result = -1;
    mm::NativeWorkspace ws;
    const float inv_k = (float)(1.0 / (double)steps);
    auto run = [&]() {
        std::string err;
        const unsigned *wx = taps_dev.get<unsigned>(), *wy = wx + y_tables;
        const mm::ClipFilterTaps taps{sx, sy, reach, wx, wy};
        const mm::ClipStore to{dst.get<unsigned char>() + out_offset, row_stride, frame_stride, bpp, floatmap};
        const mm::ClipRect rect{region_x, first_row, region_w, rows, hx0, hy0, hw, hrows, render_w, render_h};
        for (int j0 = 0; j0 < steps; j0 += steps_per_pass) {
            const int count = std::min(steps_per_pass, steps - j0);
            const bool last = j0 + count >= steps;
            const mm::ClipSamples in{subs.get<unsigned char>() + (size_t)j0 * grid * map_bytes, (int64_t)map_bytes, (int64_t)(map_bytes * grid * steps),
                                     count, j0 > 0 ? carry.get() : nullptr, last ? nullptr : carry.get()};
            if (mm::launch_filter_combine_clip(in, taps, to, rect, inv_k, frames, ws, nullptr, &err) != 0) {
                g_selftest_err = err;
                return false;
            }
        }
        return true;
    };
    do {
        if (!ok(subs.grow(all)) || !ok(dst.grow((size_t)out_bytes)) || !ok(taps_dev.grow(tables.size() * sizeof(unsigned))) ||
            (steps_per_pass < steps && !ok(carry.grow((size_t)rows * region_w * 16 * frames))))
            break;
        if (!ok(hipMemcpy(taps_dev.get(), tables.data(), tables.size() * sizeof(unsigned), hipMemcpyHostToDevice))) break;
        if (maps ? !ok(hipMemcpy(subs.get(), maps, all, hipMemcpyHostToDevice)) : !ok(hipMemsetD32((hipDeviceptr_t)subs.get(), 0x3e800000, all / 4))) break;
        if (!ok(hipMemset(dst.get(), sentinel, (size_t)out_bytes))) break;
        if (!run() || !ok(hipDeviceSynchronize())) break;
        if (out && !ok(hipMemcpy(out, dst.get(), (size_t)out_bytes, hipMemcpyDeviceToHost))) break;
        bool timed = true;
        if (rounds > 0) timed = ok(hipEventCreate(&e0)) && ok(hipEventCreate(&e1));
        for (int r = 0; r < rounds && timed; ++r) {
            float t = 0;
            timed = ok(hipEventRecord(e0, nullptr)) && run() && ok(hipEventRecord(e1, nullptr)) && ok(hipEventSynchronize(e1)) && ok(hipEventElapsedTime(&t, e0, e1));
            ms[r] = t;
        }
        if (timed) result = 0;
    } while (false);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return result;
}

}  // extern "C"
