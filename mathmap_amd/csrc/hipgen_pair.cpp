// Pair mode of the HIP generator: two pixels of a work-item evaluated in lockstep as 2-vectors.
//
// For a pixel body that is nothing but int/float arithmetic, comparisons and structured control
// flow (Mandelbrot and its relatives), the two pixels a work-item renders per loop step are
// evaluated together: every SSA value is a 2-vector (x component: the first pixel), `if`s are
// if-converted (both sides evaluated -- the slice is pure -- and the exit phis select), a `while`
// runs while either pixel is active with the loop phis frozen per pixel by a select (with lane masks: only
// at the back edges at which a lane leaves, see exit_driven_iteration).  Each component
// sees exactly the scalar kernel's operations in the scalar kernel's order.  What it buys: a gfx950
// SIMD hands a wave an issue slot every ~4 cycles, in which the wave can issue two independent vector
// instructions (2 cycles each) -- a single pixel's dependent chain uses half of that, whatever the
// occupancy (tools/pk_rate.hip: dependent v_mul/v_add 4.25 cycles per instruction at 8 waves per SIMD,
// two independent chains 2.4).  The pair's components are kept as separate scalars, so the
// instruction stream alternates between the two pixels; as v_pk_*_f32 (MM_PAIR_SCALAR=0) the same
// work issues in one 4-cycle instruction and gains much less (Mandelbrot 8192^2: 0.372 ms one pixel
// at a time, 0.360 packed, 0.313 interleaved).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <sstream>

#include "hipgen_internal.h"

namespace mm {
namespace hipgen {
namespace {

struct PairGen final : PairMode {
    PairEnv env;
    std::ostream &out;
    FilterCode &code;
    std::set<const Value *> defs;      // values defined in the pixel slice (vectors in pair mode)
    // Int values that only ever hold a truth value (results of comparisons, NOT, the literals 0 / 1 and
    // phis / copies of such): kept as a pair of bools (mm_bb), which the compiler keeps in scalar lane masks
    // where their logic is scalar arithmetic -- as ints they would cost two vector instructions per operation.
    std::set<const Value *> bools;
    std::set<const Value *> uniform;   // wave-uniform values of the loops being printed (mark_uniform)
    int ids = 0;                       // names of masks: mm_c<id>, mm_a<id>, mm_l<id>
    // exit-driven loops (exit_driven_iteration): they need lane masks; MMHIP_PAIR_EXIT=0 keeps the per-iteration selects
    const bool exit = env.knobs.pair_exit.value_or(1) && env.knobs.pair_masks.value_or(1);
    // the kernel's own result pack (emit_helpers): with the exit-driven loops, so that MMHIP_PAIR_EXIT=0 is the earlier text
    const bool pack = exit && env.knobs.pair_pack.value_or(1);
    const Stmt *split_def = nullptr;   // the uniform conjunct's defining statement, while its loop body is printed
    bool split_leave = false;          // the value with which it ends the loop
    // fused doubling (plan_fusion): with the counted back edge, so that every earlier switch gives its earlier text
    const bool fma2 = exit && env.knobs.pair_fma2.value_or(1) && env.knobs.pair_exit_tail.value_or(2) >= 2;
    // r = d + b, d = t * k: r = fma(t, k, b) and no statement for d -- unless phis that nothing reads name it (keep_d, count_uses)
    struct Fuse { const Stmt *r, *d; Primary t, b; float k; bool keep_d; };
    std::map<const Stmt *, std::vector<Fuse>> fuse_plan;            // loop -> its fused statements
    std::map<const Stmt *, const Fuse *> fusing;                    // those of the loop copies being printed fused, by r ...
    std::set<const Stmt *> fused_away;                              // ... and their d
    // the fast step (emit_pixel_loop): with the fused doubling and the kernel's own pack, so that every earlier switch gives its earlier text
    const bool step = fma2 && pack && !env.knobs.pair_peel.value_or(0) && env.knobs.pair_step.value_or(1);
    bool fast_step = false;                                         // ... and this kernel has a fused loop and a result pack (make_pair_mode)
    bool spread = false;                                            // ... whose steps the single-frame kernel deals across the launch's rows (MMHIP_PAIR_SPREAD)
    std::vector<std::string> entry_masks;                         // frame constants read as truth values: mm_ub<k> holds the lane mask of entry k

    explicit PairGen(const PairEnv &e) : env(e), out(e.out), code(e.code) {}

    bool exit_driven() const override { return exit; }
    bool is_uniform(const Value *v) const override { return uniform.count(v) > 0; }

    // ---- which bodies are covered ----
    static bool scalar_ty(Ty t) { return t == Ty::Int || t == Ty::Float; }
    static bool prim_ok(const Primary &p) {
        if (p.kind == Primary::IntConst || p.kind == Primary::FloatConst) return true;
        return p.kind == Primary::Val && scalar_ty(p.value->var->type);
    }
    static bool rhs_ok(const Rhs &r) {
        if (r.kind == Rhs::Prim) return prim_ok(r.prim);
        if (r.kind == Rhs::Internal) return r.internal == "x" || r.internal == "y";
        if (r.kind != Rhs::Op) return false;
        static const char *ok[] = {"ADD", "SUB", "MUL", "NEG", "DIV", "LESS", "LEQ", "EQ", "NOT", "sqrt"};
        bool found = false;
        for (const char *o : ok) found = found || !strcmp(r.op->cname, o);
        if (!found) return false;
        for (const Primary &a : r.args) if (!prim_ok(a)) return false;
        if (!strcmp(r.op->cname, "sqrt") && r.args[0].type() != Ty::Float) return false;
        if (!strcmp(r.op->cname, "NOT") && r.args[0].type() != Ty::Int) return false;
        return true;
    }
    bool block_ok(const Block &b) const {
        for (const Stmt *s : b) {
            if (!s->in_pixel) continue;
            switch (s->kind) {
                case Stmt::Assign:
                    if (!s->lhs || !scalar_ty(s->lhs->var->type) || !rhs_ok(s->rhs)) {
                        if (env.knobs.pair_debug)
                            fprintf(stderr, "pair mode: statement not covered (%s)\n",
                                    s->rhs.kind == Rhs::Op ? s->rhs.op->cname : s->rhs.kind == Rhs::Internal ? s->rhs.internal.c_str() : "rhs kind");
                        return false;
                    }
                    break;
                case Stmt::If:
                case Stmt::While:
                    if (s->cond.kind != Rhs::Prim || !prim_ok(s->cond.prim) || s->cond.prim.type() != Ty::Int) return false;
                    for (const Stmt *ph : s->phis) {
                        if (!ph->in_pixel) continue;
                        if (!scalar_ty(ph->lhs->var->type) || ph->rhs.kind != Rhs::Prim || ph->rhs2.kind != Rhs::Prim ||
                            !prim_ok(ph->rhs.prim) || !prim_ok(ph->rhs2.prim))
                            return false;
                    }
                    if (s->kind == Stmt::If ? !(block_ok(s->then_) && block_ok(s->else_)) : !block_ok(s->body)) return false;
                    break;
                default: break;
            }
        }
        return true;
    }
    bool eligible() const {
        if (!env.opt.fast_math_exact) return false;
        const bool force = env.knobs.pair.has_value();          // 0: never, 1: whenever the body is covered, unset: small bodies
        if (force && !*env.knobs.pair) return false;
        const int stmts = env.pixel_stmts;
        // measured at 8192^2: Mandelbrot with its parameters baked in (24 statements) 0.372 -> 0.355 ms, the generic
        // quaternion form (57 statements, four loop-carried components to keep per pixel) 0.75 -> 0.86 ms
        if (env.pixel_fetches || stmts < 4 || stmts > (force ? 400 : 40)) return false;
        const bool dbg = env.knobs.pair_debug;
        for (int i = 0; i < 4; ++i)
            if (!code.result[i] || !scalar_ty(code.result[i]->var->type)) {
                if (dbg) fprintf(stderr, "pair mode: result %d is not an int / float value\n", i);
                return false;
            }
        const bool ok = block_ok(code.body);
        if (dbg) fprintf(stderr, "pair mode: body %s (%d statements)\n", ok ? "covered" : "not covered", stmts);
        return ok;
    }

    // ---- truth values ----
    // does `d` define a truth value, given that its operands do where `operand` says so?
    template <class P> static bool truth_def(const Stmt *d, P operand) {
        if (d->kind == Stmt::Phi) return d->rhs.kind == Rhs::Prim && d->rhs2.kind == Rhs::Prim && operand(d->rhs.prim) && operand(d->rhs2.prim);
        if (d->kind != Stmt::Assign) return false;
        if (d->rhs.kind == Rhs::Prim) return operand(d->rhs.prim);
        return d->rhs.kind == Rhs::Op && is_truth_op(d->rhs.op->cname);
    }
    // a frame constant (scalar, defined in the hoisted slice) that holds a truth value
    static bool const_is_bool(const Value *v, int depth) {
        if (!v || depth > 12 || v->var->type != Ty::Int) return false;
        if (v->index < 0) return true;                      // uninitialised: reads as 0
        return v->def && truth_def(v->def, [&](const Primary &p) {
            return p.kind == Primary::IntConst ? p.i == 0 || p.i == 1 : p.kind == Primary::Val && const_is_bool(p.value, depth + 1);
        });
    }
    bool prim_bool(const Primary &p) const {
        if (p.kind == Primary::IntConst) return p.i == 0 || p.i == 1;
        if (p.kind != Primary::Val) return false;
        if (p.value->index < 0) return p.value->var->type == Ty::Int;
        if (bools.count(p.value)) return true;
        return !defs.count(p.value) && const_is_bool(p.value, 0);
    }
    void infer_bools() {
        std::vector<const Stmt *> idefs;      // the statements (assignments and phis) that define the slice's int values
        for (Value *v : env.pix_defs) {
            defs.insert(v);
            if (v->var->type == Ty::Int && v->def && v->def->lhs == v) idefs.push_back(v->def);
        }
        for (const Stmt *d : idefs) bools.insert(d->lhs);            // optimistic, then remove until stable
        for (bool changed = true; changed;) {
            changed = false;
            for (const Stmt *d : idefs)
                if (bools.count(d->lhs) && !truth_def(d, [&](const Primary &p) { return prim_bool(p); })) { bools.erase(d->lhs); changed = true; }
        }
    }
    // values read outside the body of loop `w` (statements of other blocks, other loops' phis, the results):
    // only those of w's phis, and its condition, have to keep their value once a pixel has left the loop
    void uses_outside(const Block &b, const Stmt *skip, std::set<const Value *> &uses) const {
        auto use = [&](const Primary &p) { if (p.kind == Primary::Val) uses.insert(p.value); };
        auto use_rhs = [&](const Rhs &r) { if (r.kind == Rhs::Prim) use(r.prim); for (const Primary &a : r.args) use(a); };
        for (const Stmt *s : b) {
            if (!s->in_pixel) continue;
            if (s->kind == Stmt::Assign) use_rhs(s->rhs);
            if (s->kind == Stmt::If) {
                use_rhs(s->cond);
                uses_outside(s->then_, skip, uses);
                uses_outside(s->else_, skip, uses);
                for (const Stmt *ph : s->phis) if (ph->in_pixel) { use_rhs(ph->rhs); use_rhs(ph->rhs2); }
            }
            if (s->kind == Stmt::While) {
                for (const Stmt *ph : s->phis) if (ph->in_pixel) { use_rhs(ph->rhs); if (s != skip) use_rhs(ph->rhs2); }
                if (s != skip) { use_rhs(s->cond); uses_outside(s->body, skip, uses); }
            }
        }
    }

    // ---- expressions ----
    // operand as a 2-vector of the wanted type (mm_vf / mm_vi broadcast scalars and convert int -> float)
    std::string pbool(const Primary &p) {        // operand as mm_bb
        const std::string bu = exit ? "mm_xbu(" : "mm_bu(";      // (exit-driven loops: no exec in the broadcast either)
        if (p.kind == Primary::IntConst) return bu + (p.i ? "true)" : "false)");
        if (p.kind == Primary::Val && p.value->index < 0) return bu + "false)";
        // (a uniform value that is not a literal goes through the ballot of mm_bu: a select between 64-bit constants on a
        // uniform bool is a v_cndmask_b32 pair to this compiler, and the mask would sit in vector registers)
        if (uniform.count(p.value)) return "mm_bu((bool)u" + vname(p.value) + ")";
        if (bools.count(p.value)) return vname(p.value);
        if (fast_step && !defs.count(p.value)) {      // a frame constant: its mask is made once, in front of the pixel loop (emit_pixel_loop)
            const std::string c = env.prim(p);
            size_t k = std::find(entry_masks.begin(), entry_masks.end(), c) - entry_masks.begin();
            if (k == entry_masks.size()) entry_masks.push_back(c);
            return "mm_ub" + std::to_string(k);
        }
        return "mm_tob(" + pprim(p, Ty::Int) + ")";
    }
    std::string pprim(const Primary &p, Ty want) {
        const char *w = want == Ty::Float ? "mm_vf(" : "mm_vi(";
        if (p.kind == Primary::IntConst) return std::string(w) + std::to_string(p.i) + ")";
        if (p.kind == Primary::FloatConst) return std::string(w) + float_literal(p.f) + "f)";
        if (p.value->index < 0) return std::string(w) + "0)";
        if (uniform.count(p.value))
            return std::string(w) + (p.value->var->type == Ty::Float ? "(float)u" : "(int)u") + vname(p.value) + ")";
        return std::string(w) + vname(p.value) + ")";
    }
    static Ty arith_ty(const Rhs &r) {
        for (const Primary &a : r.args) if (a.type() == Ty::Float) return Ty::Float;
        return Ty::Int;
    }
    std::string prhs(const Rhs &r, const Value *lhs) {
        const Ty lhs_ty = lhs->var->type;
        const bool as_bool = bools.count(lhs) > 0;
        if (r.kind == Rhs::Prim) return as_bool ? pbool(r.prim) : pprim(r.prim, lhs_ty);
        if (r.kind == Rhs::Internal) return r.internal == "x" ? "mm_vf(x)" : "mm_y2";
        const char *cn = r.op->cname;
        const Ty t = arith_ty(r);
        const char *op = !strcmp(cn, "ADD") ? "+" : !strcmp(cn, "SUB") ? "-" : !strcmp(cn, "MUL") ? "*" : !strcmp(cn, "LESS") ? "<"
                         : !strcmp(cn, "LEQ") ? "<=" : !strcmp(cn, "EQ") ? "==" : nullptr;
        const bool compares = op && (op[0] == '<' || op[0] == '=');
        // An int value next to a float literal: the scalar kernel's literal is a double (cc.c prints them so),
        // C computes (double)i op literal and the assignment rounds once -- (float)i first would round twice
        // for |i| >= 2^24.  Same arithmetic here, per component.
        if (op && r.args.size() == 2 && ((r.args[0].type() == Ty::Int && r.args[1].kind == Primary::FloatConst) ||
                                         (r.args[1].type() == Ty::Int && r.args[0].kind == Primary::FloatConst))) {
            auto comp = [&](const Primary &p, const char *c) {
                if (p.kind == Primary::FloatConst) return "(double)" + float_literal(p.f) + "f";
                return "(double)" + pprim(p, Ty::Int) + "." + c;
            };
            const std::string ex = comp(r.args[0], "x") + " " + op + " " + comp(r.args[1], "x");
            const std::string ey = comp(r.args[0], "y") + " " + op + " " + comp(r.args[1], "y");
            if (compares) {
                const std::string b = "mm_bl(" + ex + ", " + ey + ")";
                return as_bool ? b : "mm_vi(" + b + ")";
            }
            return "mm_pf{(float)(" + ex + "), (float)(" + ey + ")}";
        }
        if (op && !compares) return "(" + pprim(r.args[0], t) + " " + op + " " + pprim(r.args[1], t) + ")";
        if (!strcmp(cn, "NEG")) return "(-" + pprim(r.args[0], t) + ")";
        if (!strcmp(cn, "sqrt")) return "mm_sqrt2(" + pprim(r.args[0], Ty::Float) + ")";
        if (!strcmp(cn, "DIV")) {
            if (r.args[1].kind == Primary::FloatConst || r.args[1].kind == Primary::IntConst) {      // x / +-2^k = x * 2^-k, exactly
                const float c = r.args[1].kind == Primary::FloatConst ? r.args[1].f : (float)r.args[1].i;
                if (is_pow2_divisor(c)) return "(" + pprim(r.args[0], Ty::Float) + " * " + float_literal(1.0f / c) + "f)";
            }
            return "(" + pprim(r.args[0], Ty::Float) + " / " + pprim(r.args[1], Ty::Float) + ")";
        }
        // the truth-valued operators: a pair of bools; as an int (0 / 1) only if the value is used as one
        std::string b;
        const std::string notb = exit ? "mm_xnotb(" : "mm_notb(";
        if (!strcmp(cn, "NOT")) b = notb + pbool(r.args[0]) + ")";
        else if (!strcmp(cn, "EQ") && prim_bool(r.args[0]) && prim_bool(r.args[1])) {
            // b == 0 is !b, b == 1 is b, otherwise the equivalence of two truth values
            const Primary &x = r.args[0], &y = r.args[1];
            if (y.kind == Primary::IntConst) b = y.i ? pbool(x) : notb + pbool(x) + ")";
            else if (x.kind == Primary::IntConst) b = x.i ? pbool(y) : notb + pbool(y) + ")";
            else b = "mm_eqb(" + pbool(x) + ", " + pbool(y) + ")";
        } else {
            // sqrt(a) < 2^k  ->  0 <= a < 4^k, like the scalar generator (hipgen.cpp rhs)
            float kk = 0;
            const Primary *sq = sqrt_less_pow2(r, &kk);
            if (sq && env.value_visible(sq->value)) {
                const std::string a = pprim(*sq, Ty::Float), k2 = "mm_vf(" + float_literal(kk) + "f)";
                b = nonneg_or_nan(sq->value, 0) ? "mm_lt(" + a + ", " + k2 + ")"
                                                : "mm_andb(mm_lt(" + a + ", " + k2 + "), mm_le(mm_vf(0.0f), " + a + "))";
            } else {
                const char *fn = !strcmp(cn, "LESS") ? "mm_lt(" : !strcmp(cn, "LEQ") ? "mm_le(" : "mm_eq(";
                b = fn + pprim(r.args[0], t) + ", " + pprim(r.args[1], t) + ")";
            }
        }
        return as_bool ? b : "mm_vi(" + b + ")";
    }
    std::string pair_ctype(const Value *v) const {      // the C type of a value's pair
        return bools.count(v) ? "mm_bb" : v->var->type == Ty::Float ? "mm_pf" : "mm_pi";
    }
    std::string pval_as(const Primary &p, const Value *lhs) {      // operand in the representation of `lhs`
        return bools.count(lhs) ? pbool(p) : pprim(p, lhs->var->type);
    }

    // ---- wave-uniform values inside a loop ----
    // A loop phi that starts from a literal or a frame constant
    // and is stepped by one -- `n = n + 1`, the iteration counter of every escape-time filter -- holds the same
    // value in every lane and in both pixels for as long as they are in the loop, and so does everything
    // computed from such values and loop-invariant scalars alone (`n + 1`, `n < 31`).  Those are kept as plain
    // scalars (the compiler holds them in SGPRs and evaluates them on the scalar unit: uniform inside a loop
    // with divergent exits) instead of as per-lane pairs; the per-pixel copy a phi needs after the loop is one
    // select per iteration instead of an add, a compare and a select.  Values of pixels that have left the loop
    // are don't-cares inside it, exactly as before.
    bool invariant_scalar(const Primary &p) const {
        if (p.kind == Primary::IntConst || p.kind == Primary::FloatConst) return true;
        if (p.kind != Primary::Val) return false;
        return p.value->index < 0 || !defs.count(p.value);          // uninitialised (0) or a frame constant
    }
    bool uniform_operand(const Primary &p) const {
        return invariant_scalar(p) || (p.kind == Primary::Val && uniform.count(p.value));
    }
    void mark_uniform(const Block &b) {      // forward pass over a loop body (SSA: definitions precede uses)
        for (const Stmt *s : b) {
            if (!s->in_pixel) continue;
            if (s->kind == Stmt::Assign && s->rhs.kind != Rhs::Internal) {
                bool ok = s->rhs.kind == Rhs::Prim ? uniform_operand(s->rhs.prim) : s->rhs.kind == Rhs::Op;
                if (ok && s->rhs.kind == Rhs::Op)
                    for (const Primary &a : s->rhs.args) ok = ok && uniform_operand(a);
                // a plain copy of an invariant scalar stays a broadcast (nothing to gain); ops on uniform values do not
                if (ok && s->rhs.kind == Rhs::Prim && !(s->rhs.prim.kind == Primary::Val && uniform.count(s->rhs.prim.value))) ok = false;
                // truth values stay pairs of bools built from the (broadcast) uniform operands: the compiler evaluates such a
                // comparison on the scalar unit anyway, and keeps the pair in lane masks only in that form (checked in the ISA).
                // With lane masks that no longer holds -- the ballot of a uniform comparison is a v_cmp per iteration -- so the
                // exit-driven loops keep them as scalar bools, broadcast with mm_bu where a pair is wanted.
                if (ok && bools.count(s->lhs) && !exit) ok = false;
                if (ok) uniform.insert(s->lhs);
            } else if (s->kind == Stmt::If) {
                mark_uniform(s->then_);
                mark_uniform(s->else_);
            }
        }
    }
    // the phis of `w` that are uniform induction variables; marks them and what follows from them
    std::vector<const Stmt *> find_uniform_ivs(const Stmt *w) {
        std::vector<const Stmt *> ivs;
        if (env.knobs.pair_no_uniform) return ivs;
        for (const Stmt *ph : w->phis) {
            if (!ph->in_pixel || ph->rhs.kind != Rhs::Prim || ph->rhs2.kind != Rhs::Prim) continue;
            if (!scalar_ty(ph->lhs->var->type) || bools.count(ph->lhs)) continue;
            if (!invariant_scalar(ph->rhs.prim) || ph->rhs2.prim.kind != Primary::Val) continue;
            const Stmt *d = ph->rhs2.prim.value->def;
            if (!d || d->kind != Stmt::Assign || d->parent != w || d->rhs.kind != Rhs::Op || d->rhs.args.size() != 2) continue;
            const char *cn = d->rhs.op->cname;
            const Primary &a0 = d->rhs.args[0], &a1 = d->rhs.args[1];
            const bool self0 = a0.kind == Primary::Val && a0.value == ph->lhs, self1 = a1.kind == Primary::Val && a1.value == ph->lhs;
            const bool step = (!strcmp(cn, "ADD") && ((self0 && invariant_scalar(a1)) || (self1 && invariant_scalar(a0)))) ||
                              (!strcmp(cn, "SUB") && self0 && invariant_scalar(a1));
            if (!step) continue;
            ivs.push_back(ph);
            uniform.insert(ph->lhs);
        }
        if (!ivs.empty()) mark_uniform(w->body);
        return ivs;
    }

    // ---- the uniform conjunct of an exit-driven loop's condition (see exit_driven_iteration) ----
    struct Body {                                          // what find_split needs to know about a loop body
        std::set<const Value *> defs;
        std::map<const Value *, const Stmt *> if_of;      // exit phi of an `if` -> the if
        std::vector<const Stmt *> order;                  // assignments and if-phis in program order
        bool nested_loop = false;
    };
    void scan_body(const Block &b, Body &pb) const {
        for (const Stmt *s : b) {
            if (!s->in_pixel) continue;
            if (s->kind == Stmt::Assign) { pb.defs.insert(s->lhs); pb.order.push_back(s); }
            if (s->kind == Stmt::While) pb.nested_loop = true;
            if (s->kind == Stmt::If) {
                scan_body(s->then_, pb);
                scan_body(s->else_, pb);
                for (const Stmt *ph : s->phis)
                    if (ph->in_pixel) { pb.defs.insert(ph->lhs); pb.if_of[ph->lhs] = s; pb.order.push_back(ph); }
            }
        }
    }
    // three-valued truth of `p` (0, 1, -1: unknown) when the value `l` is `lv` and nothing else is known
    int eval3(const Primary &p, const Body &pb, const Value *l, int lv, int depth = 0) const {
        if (p.kind == Primary::IntConst) return p.i == 0 ? 0 : p.i == 1 ? 1 : -1;
        if (p.kind != Primary::Val || depth > 32) return -1;
        if (p.value->index < 0) return 0;
        if (p.value == l) return lv;
        if (!pb.defs.count(p.value) || !bools.count(p.value)) return -1;
        const Stmt *d = p.value->def;
        if (!d) return -1;
        if (d->kind == Stmt::Phi) {
            auto it = pb.if_of.find(p.value);
            if (it == pb.if_of.end() || d->rhs.kind != Rhs::Prim || d->rhs2.kind != Rhs::Prim) return -1;
            const Primary &cp = it->second->cond.prim;
            const int c = eval3(cp, pb, l, lv, depth + 1);
            // `c ? c : b` is `c ? 1 : b`, `c ? a : c` is `c ? a : 0`
            const bool same1 = cp.kind == Primary::Val && d->rhs.prim.kind == Primary::Val && d->rhs.prim.value == cp.value && bools.count(cp.value);
            const bool same2 = cp.kind == Primary::Val && d->rhs2.prim.kind == Primary::Val && d->rhs2.prim.value == cp.value && bools.count(cp.value);
            const int a = same1 ? 1 : eval3(d->rhs.prim, pb, l, lv, depth + 1);
            const int b = same2 ? 0 : eval3(d->rhs2.prim, pb, l, lv, depth + 1);
            if (c == 1) return a;
            if (c == 0) return b;
            return a == b ? a : -1;
        }
        if (d->kind != Stmt::Assign) return -1;
        if (d->rhs.kind == Rhs::Prim) return eval3(d->rhs.prim, pb, l, lv, depth + 1);
        if (d->rhs.kind != Rhs::Op) return -1;
        const char *cn = d->rhs.op->cname;
        if (!strcmp(cn, "NOT")) { const int x = eval3(d->rhs.args[0], pb, l, lv, depth + 1); return x < 0 ? -1 : !x; }
        if (!strcmp(cn, "EQ") && prim_bool(d->rhs.args[0]) && prim_bool(d->rhs.args[1])) {
            const int x = eval3(d->rhs.args[0], pb, l, lv, depth + 1), y = eval3(d->rhs.args[1], pb, l, lv, depth + 1);
            return x < 0 || y < 0 ? -1 : x == y;
        }
        return -1;
    }
    // the uniform conjunct of w's condition, if there is one that may be split off; `leave`: the value with which it ends the loop
    const Stmt *find_split(const Stmt *w, const std::set<const Value *> &outside, bool &leave) const {
        if (w->cond.prim.kind != Primary::Val) return nullptr;
        Body pb;
        scan_body(w->body, pb);
        if (pb.nested_loop) return nullptr;
        // the condition at the back edge: the condition phi's next value
        const Stmt *cph = nullptr;
        for (const Stmt *ph : w->phis) if (ph->in_pixel && ph->lhs == w->cond.prim.value) cph = ph;
        if (!cph || cph->rhs2.kind != Rhs::Prim) return nullptr;
        for (const Stmt *d : pb.order) {
            if (d->kind != Stmt::Assign || !uniform.count(d->lhs) || !bools.count(d->lhs) || d->rhs.kind != Rhs::Op) continue;
            if (!is_truth_op(d->rhs.op->cname) || d->rhs.args.size() != 2) continue;      // a comparison (NOT has one operand)
            if (d->rhs.args[0].type() != Ty::Int || d->rhs.args[1].type() != Ty::Int) continue;
            for (int lv = 0; lv < 2; ++lv) {
                if (eval3(cph->rhs2.prim, pb, d->lhs, lv) != 0) continue;
                // what depends on the conjunct must not reach a phi that is read after the loop
                std::set<const Value *> dep{d->lhs};
                auto in = [&](const Primary &p) { return p.kind == Primary::Val && dep.count(p.value) > 0; };
                for (const Stmt *q : pb.order) {
                    bool dp = false;
                    if (q->kind == Stmt::Assign) { if (q->rhs.kind == Rhs::Prim) dp = in(q->rhs.prim); for (const Primary &a : q->rhs.args) dp = dp || in(a); }
                    else dp = in(pb.if_of.at(q->lhs)->cond.prim) || in(q->rhs.prim) || in(q->rhs2.prim);
                    if (dp) dep.insert(q->lhs);
                }
                bool ok = true;
                for (const Stmt *ph : w->phis)
                    if (ph->in_pixel && outside.count(ph->lhs) && in(ph->rhs2.prim)) ok = false;
                if (!ok) continue;
                leave = lv != 0;
                return d;
            }
        }
        return nullptr;
    }
    // operand of the back edge's scalar comparison: a literal, or the uniform value in a scalar register
    bool tail_operand(const Primary &p, std::string &text, std::vector<std::string> &inputs, int first_input) {
        if (p.kind == Primary::IntConst) { text = std::to_string(p.i); return true; }
        if (p.kind != Primary::Val) return false;
        text = "%" + std::to_string(first_input + (int)inputs.size());
        inputs.push_back("__builtin_amdgcn_readfirstlane((int)(" + env.prim(p) + "))");
        return true;
    }

    // ---- loops ----
    struct Loop {
        Stmt *s;
        std::string ind, a;                       // indentation; the mask of the pixels still in the loop (mm_bb)
        std::set<const Value *> outside;          // phis that are read after the loop
        std::vector<const Stmt *> ivs;            // uniform induction variables: a scalar twin, read inside the loop instead of the pair
        std::vector<std::pair<const Stmt *, std::string>> exit_copy;      // exit-driven: a phi of `outside` and the name of its exit copy
        // counted back edge (plan_counted): the uniform bound as the carry of one s_add_u32
        bool counted = false;
        unsigned count_step = 0;                  // what the counter gains per trip: |step| of the induction variable
        const Stmt *count_iv = nullptr;           // the induction variable whose scalar twin is computed from the counter, if any
        std::string count_twin;                   // ... and the expression that does so
        bool is_iv(const Stmt *ph) const { return std::find(ivs.begin(), ivs.end(), ph) != ivs.end(); }
    };
    // Back edge: the phis take their next values -- a parallel copy, temporaries first -- and the induction variables'
    // scalar twins theirs.  `select`: a phi that is read after the loop keeps its value once its pixel has left;
    // without it the pairs of the induction variables are not kept up at all.
    void step_phis(const Loop &w, const std::string &I, bool select) {
        std::vector<Stmt *> phis;
        for (Stmt *ph : w.s->phis) if (ph->in_pixel && (select || !w.is_iv(ph))) phis.push_back(ph);
        for (size_t k = 0; k < phis.size(); ++k) {
            const std::string nv = pval_as(phis[k]->rhs2.prim, phis[k]->lhs);
            out << I << "const " << pair_ctype(phis[k]->lhs) << " " << w.a << "_n" << k << " = "
                << (select && w.outside.count(phis[k]->lhs) ? "mm_sel2(" + w.a + ", " + nv + ", " + vname(phis[k]->lhs) + ")" : nv) << ";\n";
        }
        for (size_t k = 0; k < phis.size(); ++k) out << I << vname(phis[k]->lhs) << " = " << w.a << "_n" << k << ";\n";
        for (const Stmt *ph : w.ivs)
            if (ph != w.count_iv) out << I << "u" << vname(ph->lhs) << " = " << env.prim(ph->rhs2.prim) << ";\n";
    }
    // Counted back edge (MMHIP_PAIR_EXIT_TAIL unset or 2).  The uniform conjunct compares an int that gains a literal step s per
    // trip -- an induction variable (its value before the step) or its stepped value -- with a loop-invariant bound, and the
    // loop runs while the comparison holds (LESS, LEQ and their negations) or until the two are equal (the negation of EQ, s =
    // +-1).  Then the back edge at which it ends the loop is known when the loop is entered: with o the operand's value one
    // step before the first test and D the distance it has to cover -- `o < B`, s > 0: D = B - o; `o <= B`: one more; `B < o`,
    // s < 0: D = o - B; ... -- it is the first at which trips * |s| >= D.  A counter k = 2^32 - D that gains |s| per trip wraps
    // around exactly there, so one s_add_u32 steps it and leaves the bound's verdict in SCC (its carry), where the compare-and-mask
    // tail steps the induction variable and compares (s_add_i32, s_cmp); and since nothing clobbers SCC in between, one s_cselect_b64
    // folds the verdict into the `left` word (-1: every lane leaves) where that tail builds a mask and ORs it in.  D <= 0 --
    // the comparison fails before the first step: it fails at the first test as well, the operand moves away -- counts as 1.
    // A literal distance that does not fit the counter (above 2^32 - 1) keeps the compare-and-mask tail; a run-time distance is
    // clamped to 2^32 - 1 there (more than four billion trips: not reachable in practice).
    // In the exit block k < |s| says that the counter has wrapped.  (An operand that overflows int before it reaches the
    // bound is undefined in the scalar kernel's C; here the loop then ends where the exact sum reaches the bound.)
    // With literal initial value and bound the induction variable's scalar twin is a function of k, u = init +- (k - k0): it is
    // computed from k at the top of the body -- for nothing if only the bound reads it -- and is not stepped on its own.
    // Anything else (a bound on a lagging copy, `==` as the running condition, a step that is no literal or points away from
    // the bound) keeps the compare-and-mask tail.
    // The relation under which a loop with the uniform conjunct `a0 CN a1` runs, the operand on side `side` advancing by `step`:
    // the comparison itself, or -- `leave`: the conjunct's truth ends the loop -- its negation, which swaps the sides and turns
    // `<` into `<=` (!(a < b) is b <= a).  Covered: the operand moves towards the bound of `<` (`inclusive`: `<=`), or, for the
    // negation of `==`, by +-1:
    //   o <  B / o <= B   operand left    up          B <  o / B <= o   operand right   down          o != B   either side   +-1
    static bool counted_relation(const char *cn, bool leave, int side, long step, bool &inclusive) {
        if (!strcmp(cn, "EQ")) { inclusive = false; return leave && (step == 1 || step == -1); }
        const bool advancing_left = leave ? side == 1 : side == 0;
        inclusive = leave ? !strcmp(cn, "LESS") : !strcmp(cn, "LEQ");
        return advancing_left ? step > 0 : step < 0;
    }
    void plan_counted(Loop &w, const std::string &l) {
        if (env.knobs.pair_exit_tail.value_or(2) < 2) return;
        bool leave = false;
        const Stmt *split = find_split(w.s, w.outside, leave);
        if (!split) return;
        const char *cn = split->rhs.op->cname;
        const bool eq = !strcmp(cn, "EQ");
        // the advancing operand: which side, which induction variable, its step, its value one step before the first test
        int side = -1;
        const Stmt *iv = nullptr;
        long step = 0;
        bool stepped = false;
        for (int i = 0; i < 2 && side < 0; ++i) {
            const Primary &p = split->rhs.args[i];
            if (p.kind != Primary::Val) continue;
            for (const Stmt *ph : w.ivs) {
                if (ph->lhs->var->type != Ty::Int) continue;
                const Stmt *d = ph->rhs2.prim.value->def;
                const bool self0 = d->rhs.args[0].kind == Primary::Val && d->rhs.args[0].value == ph->lhs;
                const Primary &c = d->rhs.args[self0 ? 1 : 0];
                if (c.kind != Primary::IntConst || (p.value != ph->lhs && p.value != d->lhs)) continue;
                side = i; iv = ph; stepped = p.value == d->lhs;
                step = !strcmp(d->rhs.op->cname, "SUB") ? -(long)c.i : (long)c.i;
            }
        }
        if (side < 0 || step == 0 || step > 0x7fffffffL || step < -0x7fffffffL) return;
        const Primary &bound = split->rhs.args[1 - side], &init = iv->rhs.prim;
        if (!invariant_scalar(bound) || bound.type() != Ty::Int || init.type() != Ty::Int) return;
        bool inclusive = false;
        if (!counted_relation(cn, leave, side, step, inclusive)) return;
        const bool up = step > 0;
        const long pre = stepped ? 0 : -step;              // the operand one step before the first test: init + pre
        auto lit = [](const Primary &p, long &v) {
            if (p.kind == Primary::IntConst) { v = p.i; return true; }
            if (p.kind == Primary::Val && p.value->index < 0) { v = 0; return true; }
            return false;
        };
        long iv0 = 0, b0 = 0;
        const std::string k = l + "_k";
        if (lit(init, iv0) && lit(bound, b0)) {
            long d = up ? b0 - (iv0 + pre) : (iv0 + pre) - b0;
            if (eq) d &= 0xffffffffL; else d += inclusive ? 1 : 0;
            if (!eq && d > 0xffffffffL) return;      // (more trips than the counter holds: the compare-and-mask tail)
            const bool exact = eq || d > 0;
            if (!exact) d = 1;
            const unsigned k0 = 0u - (unsigned)d;
            out << w.ind << "unsigned " << k << " = " << k0 << "u;\n";
            if (exact) {
                w.count_iv = iv;
                const unsigned c = up ? (unsigned)iv0 - k0 : (unsigned)iv0 + k0;
                w.count_twin = "(int)(" + std::to_string(c) + "u " + (up ? "+ " : "- ") + k + ")";
            }
        } else {
            uniform.erase(iv->lhs);       // the initial value is printed with the ordinary names
            const std::string o = "((long)(" + env.prim(init) + ") + " + std::to_string(pre) + "l)", b = "(long)(" + env.prim(bound) + ")";
            uniform.insert(iv->lhs);
            const std::string d = (up ? b + " - " + o : o + " - " + b) + (inclusive ? " + 1l" : "");
            out << w.ind << "const long " << k << "_d = " << d << ";\n";
            out << w.ind << "unsigned " << k << " = __builtin_amdgcn_readfirstlane(0u - (unsigned)("
                << (eq ? k + "_d" : k + "_d <= 0l ? 1l : " + k + "_d > 0xffffffffl ? 0xffffffffl : " + k + "_d") << "));\n";
        }
        w.counted = true;
        w.count_step = (unsigned)(up ? step : -step);
    }
    // Per-iteration selects (no lane masks, or MMHIP_PAIR_EXIT=0): one iteration and its back edge.
    void selecting_iteration(const Loop &w) {
        Stmt *s = w.s;
        const std::string &ind = w.ind, &a = w.a;
        stmts(s->body, ind + "  ", a);
        // A phi that is read after the loop, and the loop condition, keep their value once their pixel has left the
        // loop (after the loop a phi is read through this per-pixel copy); the others may run on.
        step_phis(w, ind + "  ", true);
        out << ind << "  " << a << " = mm_andb(" << a << ", " << pbool(s->cond.prim) << ");\n";
    }
    // Exit-driven loops (MM_PAIR_EXIT, lane masks only).
    // A pixel's `active` bit is monotone: it clears once.  The value a loop phi has after the loop is the value it
    // had at the back edge at which its pixel's bit cleared, so nothing has to be selected at any other back edge.
    // The loop runs in two levels: the inner do-while is the likely path (the phis' running copies take their next
    // values unconditionally, `left = active & ~cond` is two s_andn2_b64, one scalar test), the outer level is the
    // exit block: every phi that is read after the loop has an exit copy, initialised with the phi's initial value
    // and written there for the lanes in `left`, which are then cleared from `active`.  Every lane that ever was
    // active is written exactly once, at the back edge and with the value of the last select that changed it in
    // the per-iteration form, so the results are the same bits.  (Two levels, one exit each: with two exits from
    // one loop the compiler's control-flow passes rebuild the conditions as lane masks and copy the phis' registers
    // at the back edge; profiles/r05_pair_loop_isa.txt has the counts of the shapes tried.)
    //
    // A wave-uniform conjunct of the loop condition -- `n < 31` of an escape-time loop: a comparison of uniform ints
    // such that the condition is false for every lane once it has one value -- is not ANDed into the masks at all:
    // inside the loop its name is bound to the value it has while the loop runs (the compiler folds the logic built
    // on it), the comparison itself is made at the back edge on the scalar unit, and when it ends the loop every
    // active lane leaves.  Only taken when no phi that is read after the loop depends on the conjunct (in the last
    // iteration its name holds the wrong value).  Looking at one iteration is enough for that: in every iteration but the
    // last the bound name *is* the conjunct's value, so whatever the phis carry into a later iteration is right; wrong
    // values only arise in the last iteration, no iteration follows it, and what it leaves behind is read through the
    // exit copies alone -- whose next values the scan has shown not to depend on the conjunct.  The conjunct's own
    // operands are read at the end of the body, before the phis step.  The back edge is one asm statement then: left to itself
    // (MMHIP_PAIR_EXIT_TAIL=0) the compiler combines the two tests as lane masks (s_cselect_b64, s_and_b64 with exec, branch on
    // vcc: 12 scalar instructions per iteration); comparing and masking in the statement (s_cmp, s_cselect_b64, two s_andn2_b64,
    // two s_or_b64: MMHIP_PAIR_EXIT_TAIL=1, and every bound plan_counted does not cover) the loop needs 9; counted (the default
    // where plan_counted applies) it needs 7.
    void exit_driven_iteration(const Loop &w, const std::string &l) {
        Stmt *s = w.s;
        const std::string &ind = w.ind, &a = w.a, I2 = ind + "    ";
        bool leave = false;
        const Stmt *split = find_split(s, w.outside, leave);
        // the back edge's scalar comparison as one asm statement: its operands
        std::vector<std::string> tail_inputs;
        std::string tail_o0, tail_o1;
        const bool asm_tail = split && !w.counted && env.knobs.pair_exit_tail.value_or(1) &&
                              !(split->rhs.args[0].kind == Primary::IntConst && split->rhs.args[1].kind == Primary::IntConst) &&
                              tail_operand(split->rhs.args[0], tail_o0, tail_inputs, 8) && tail_operand(split->rhs.args[1], tail_o1, tail_inputs, 8);
        out << ind << "  mm_bb " << l << ";"
            << (w.counted ? " unsigned long " + l + "_t;" : asm_tail ? " unsigned long " + l + "_u, " + l + "_t;" : split ? " bool " + l + "_b;" : "") << "\n";
        out << ind << "  do {\n";
        if (w.count_iv) out << I2 << "const int u" << vname(w.count_iv->lhs) << " = " << w.count_twin << ";\n";
        const Stmt *outer_split = split_def;
        const bool outer_leave = split_leave;
        split_def = split;
        split_leave = leave;
        stmts(s->body, I2, a);
        split_def = outer_split;
        split_leave = outer_leave;
        // The conjunct stands for a statement of the body: its operands are read here, before the phis and the induction
        // variables take their next values (an operand may be such a phi: `m = n; n = n + 1` with `m < 6` as the bound).
        if (asm_tail)
            for (size_t i = 0; i < tail_inputs.size(); ++i) {
                out << I2 << "const int " << l << "_o" << i << " = " << tail_inputs[i] << ";\n";
                tail_inputs[i] = l + "_o" + std::to_string(i);
            }
        else if (split && !w.counted)
            out << I2 << l << "_b = (bool)(" << env.rhs(split) << ") == " << (leave ? "true" : "false") << ";\n";
        step_phis(w, I2, false);      // nothing selected
        // lanes that leave at this back edge
        const std::string c = pbool(s->cond.prim);
        const std::string lx = a + ".x & ~" + c + ".x", ly = a + ".y & ~" + c + ".y";
        if (w.counted) {
            // left = active & ~cond; _t = left.x | left.y, or all ones when the counter wraps: the bound ends the loop
            out << I2 << "const mm_bb " << l << "_c = " << c << ";\n";
            out << I2 << "asm(\"s_andn2_b64 %0, %4, %6\\n\\ts_andn2_b64 %1, %5, %7\\n\\ts_or_b64 %3, %0, %1\\n\\ts_add_u32 %2, %2, " << w.count_step
                << "\\n\\ts_cselect_b64 %3, -1, %3\"\n"
                << I2 << "    : \"=&s\"(" << l << ".x), \"=&s\"(" << l << ".y), \"+s\"(" << l << "_k), \"=&s\"(" << l << "_t)\n"
                << I2 << "    : \"s\"(" << a << ".x), \"s\"(" << a << ".y), \"s\"(" << l << "_c.x), \"s\"(" << l << "_c.y) : \"scc\");\n";
            out << ind << "  } while (" << l << "_t == 0);\n";
            out << ind << "  if (" << l << "_k < " << w.count_step << "u) " << l << " = " << a << ";      // the counter has wrapped: every active lane leaves\n";
            if (w.count_iv) out << ind << "  u" << vname(w.count_iv->lhs) << " = " << w.count_twin << ";\n";
        } else if (asm_tail) {
            // SCC = the conjunct; _u = all ones when it ends the loop; left = active & ~cond; _t = _u | left.x | left.y
            const char *cn = split->rhs.op->cname;
            const char *cmp = !strcmp(cn, "LESS") ? "s_cmp_lt_i32" : !strcmp(cn, "LEQ") ? "s_cmp_le_i32" : "s_cmp_eq_i32";
            out << I2 << "const mm_bb " << l << "_c = " << c << ";\n";
            out << I2 << "asm(\"" << cmp << " " << tail_o0 << ", " << tail_o1 << "\\n\\ts_cselect_b64 %2, " << (leave ? "-1, 0" : "0, -1")
                << "\\n\\ts_andn2_b64 %0, %4, %6\\n\\ts_andn2_b64 %1, %5, %7\\n\\ts_or_b64 %3, %2, %0\\n\\ts_or_b64 %3, %3, %1\"\n"
                << I2 << "    : \"=&s\"(" << l << ".x), \"=&s\"(" << l << ".y), \"=&s\"(" << l << "_u), \"=&s\"(" << l << "_t)\n"
                << I2 << "    : \"s\"(" << a << ".x), \"s\"(" << a << ".y), \"s\"(" << l << "_c.x), \"s\"(" << l << "_c.y)";
            for (const std::string &in : tail_inputs) out << ", \"s\"(" << in << ")";
            out << " : \"scc\");\n";
            out << ind << "  } while (" << l << "_t == 0);\n";
            // the uniform conjunct has ended the loop: every lane that was still active leaves
            out << ind << "  " << l << ".x |= " << a << ".x & " << l << "_u; " << l << ".y |= " << a << ".y & " << l << "_u;\n";
        } else if (split) {
            out << I2 << l << " = mm_bb{" << lx << ", " << ly << "};\n";
            out << ind << "  } while (!" << l << "_b && (" << l << ".x | " << l << ".y) == 0);\n";
            out << ind << "  if (" << l << "_b) " << l << " = " << a << ";      // the uniform conjunct has ended the loop: every active lane leaves\n";
        } else {
            out << I2 << l << " = mm_bb{" << lx << ", " << ly << "};\n";
            out << ind << "  } while ((" << l << ".x | " << l << ".y) == 0);\n";
        }
        // exit block: the phis hold their next values; a uniform induction variable's is its scalar twin's
        for (const auto &e : w.exit_copy) {
            std::string nv = vname(e.first->lhs);
            if (w.is_iv(e.first)) nv = e.first->lhs->var->type == Ty::Float ? "mm_vf((float)u" + nv + ")" : "mm_vi(mm_s2v((int)u" + nv + "))";
            out << ind << "  " << e.second << " = mm_sel2(" << l << ", " << nv << ", " << e.second << ");\n";
        }
        out << ind << "  " << a << ".x &= ~" << l << ".x; " << a << ".y &= ~" << l << ".y;\n";
    }
    // ---- fused doubling (MMHIP_PAIR_FMA2) ----
    // The imaginary part of an escape-time loop is `t = x * y; d = t + t; y' = d + b`.  Doubling is exact, so the sum rounds
    // once: it is fma(t, 2, b), one instruction for two, except where t + t overflows -- the two-step form then gives an
    // infinity whatever b is, the fused form the rounded 2t + b, which is finite again only for |b| > 2^103 (the smallest
    // product that overflows is 2^128, the largest sum that rounds to a finite float lies below 2^128 - 2^103).  The same
    // holds for every multiplier 2^k, k >= 1: scaling up is exact for denormal t as well (scaling down would not be), a zero
    // product keeps t's sign and meets b under the same addition rule, and a NaN operand gives NaN either way.
    // Fused: a float statement `r = d + b` / `r = b + d` of a loop in exit-driven form, where d is defined in the same block of
    // that loop's body as t + t or t times a literal 2^k, is read by nothing else (not by a live phi either: the exit copies
    // read those), and b comes from outside the loop: a literal (of at most 2^102: no guard), a frame constant or a pixel value of
    // an enclosing block.  Where an addend is not a literal the loop is printed twice (fused_loop) under a guard that is
    // evaluated where the loop is entered.  Nothing else is fused: not x * x + y * y (a product that is not exact), not an
    // addend that changes from trip to trip, not an int.
    //
    // Uses of every value: by assignments, conditions and the results, and by the phis whose own value is live.  A loop nested
    // in a loop has a phi for every temporary of its body (the value left by the outer loop's last trip meets the new one);
    // nothing reads those, they form cycles among themselves, and the compiler drops them: `dead` counts what only they read.
    struct Uses { std::map<const Value *, int> live, dead; };
    template <class F> static void each_phi(const Block &b, F f) {
        for (const Stmt *s : b) {
            for (const Stmt *ph : s->phis) f(ph);
            each_phi(s->then_, f);
            each_phi(s->else_, f);
            each_phi(s->body, f);
        }
    }
    static void count_roots(const Block &b, std::map<const Value *, int> &n) {
        auto use = [&](const Primary &p) { if (p.kind == Primary::Val) ++n[p.value]; };
        auto use_rhs = [&](const Rhs &r) { if (r.kind == Rhs::Prim) use(r.prim); for (const Primary &a : r.args) use(a); };
        for (const Stmt *s : b) {
            if (s->kind == Stmt::Assign) use_rhs(s->rhs);
            if (s->kind == Stmt::If || s->kind == Stmt::While) use_rhs(s->cond);
            count_roots(s->then_, n);
            count_roots(s->else_, n);
            count_roots(s->body, n);
        }
    }
    Uses count_uses() const {
        Uses u;
        count_roots(code.body, u.live);
        for (int i = 0; i < 4; ++i) if (code.result[i]) ++u.live[code.result[i]];
        std::vector<const Stmt *> phis;
        each_phi(code.body, [&](const Stmt *ph) { phis.push_back(ph); });
        std::set<const Stmt *> live_phis;
        auto operands = [](const Stmt *ph, auto f) {
            for (const Rhs *r : {&ph->rhs, &ph->rhs2}) if (r->kind == Rhs::Prim && r->prim.kind == Primary::Val) f(r->prim.value);
        };
        for (bool changed = true; changed;) {
            changed = false;
            for (const Stmt *ph : phis)
                if (!live_phis.count(ph) && u.live.count(ph->lhs)) {
                    live_phis.insert(ph);
                    operands(ph, [&](const Value *v) { ++u.live[v]; });
                    changed = true;
                }
        }
        for (const Stmt *ph : phis)
            if (!live_phis.count(ph)) operands(ph, [&](const Value *v) { ++u.dead[v]; });
        return u;
    }
    static void defined_in(const Block &b, std::set<const Value *> &d) {
        for (const Stmt *s : b) {
            if (s->kind == Stmt::Assign) d.insert(s->lhs);
            for (const Stmt *ph : s->phis) d.insert(ph->lhs);
            defined_in(s->then_, d);
            defined_in(s->else_, d);
            defined_in(s->body, d);
        }
    }
    static int count_stmts(const Block &b) {      // like the generator's pixel_stats
        int n = 0;
        for (const Stmt *s : b)
            if (s->in_pixel) n += 1 + count_stmts(s->then_) + count_stmts(s->else_) + count_stmts(s->body);
        return n;
    }
    static bool pow2_multiplier(const Primary &p, float &k) {      // a literal 2^k, k >= 1
        if (p.kind != Primary::IntConst && p.kind != Primary::FloatConst) return false;
        k = p.kind == Primary::IntConst ? (float)p.i : p.f;
        if (!(k >= 2.0f) || k > 0x1p127f) return false;
        unsigned bits;
        memcpy(&bits, &k, 4);
        return (bits & 0x7fffffu) == 0;
    }
    // d = t + t, 2^k * t or t * 2^k in floats
    static bool doubling(const Stmt *d, Primary &t, float &k) {
        if (d->kind != Stmt::Assign || !d->in_pixel || d->lhs->var->type != Ty::Float || d->rhs.kind != Rhs::Op || d->rhs.args.size() != 2) return false;
        const Primary &a0 = d->rhs.args[0], &a1 = d->rhs.args[1];
        auto fval = [](const Primary &p) { return p.kind == Primary::Val && p.value->var->type == Ty::Float; };
        if (!strcmp(d->rhs.op->cname, "ADD") && fval(a0) && fval(a1) && a0.value == a1.value) { t = a0; k = 2.0f; return true; }
        if (strcmp(d->rhs.op->cname, "MUL")) return false;
        if (fval(a0) && pow2_multiplier(a1, k)) { t = a0; return true; }
        if (fval(a1) && pow2_multiplier(a0, k)) { t = a1; return true; }
        return false;
    }
    void plan_block(const Block &b, const std::set<const Value *> &in_loop, const Uses &uses, std::vector<Fuse> &fs) const {
        for (const Stmt *r : b) {
            if (!r->in_pixel) continue;
            if (r->kind == Stmt::If) { plan_block(r->then_, in_loop, uses, fs); plan_block(r->else_, in_loop, uses, fs); }
            if (r->kind != Stmt::Assign || r->lhs->var->type != Ty::Float || uniform.count(r->lhs)) continue;
            if (r->rhs.kind != Rhs::Op || strcmp(r->rhs.op->cname, "ADD") || r->rhs.args.size() != 2) continue;
            for (int i = 0; i < 2; ++i) {
                const Primary &dp = r->rhs.args[i], &bp = r->rhs.args[1 - i];
                if (dp.kind != Primary::Val || dp.value->index < 0 || !dp.value->def || dp.value->def->lhs != dp.value) continue;
                const Stmt *d = dp.value->def;
                Fuse f{r, d, Primary(), bp, 0.0f, uses.dead.count(d->lhs) > 0};
                if (std::find(b.begin(), b.end(), d) == b.end() || uniform.count(d->lhs) || !doubling(d, f.t, f.k)) continue;
                const auto n = uses.live.find(d->lhs);
                if (n == uses.live.end() || n->second != 1) continue;
                if (bp.kind == Primary::FloatConst) { if (!(__builtin_fabsf(bp.f) <= 0x1p102f)) continue; }
                else if (bp.kind == Primary::Val) { if (bp.value->var->type != Ty::Float || in_loop.count(bp.value)) continue; }
                else if (bp.kind != Primary::IntConst) continue;
                fs.push_back(f);
                break;
            }
        }
    }
    void plan_loops(const Block &b, const Uses &uses) {
        for (const Stmt *s : b) {
            if (!s->in_pixel) continue;
            if (s->kind == Stmt::If) { plan_loops(s->then_, uses); plan_loops(s->else_, uses); }
            if (s->kind != Stmt::While) continue;
            const std::vector<const Stmt *> ivs = find_uniform_ivs(s);      // as while_loop will: uniform statements are scalar text
            std::set<const Value *> in_loop;
            for (const Stmt *ph : s->phis) in_loop.insert(ph->lhs);
            defined_in(s->body, in_loop);
            std::vector<Fuse> fs;
            plan_block(s->body, in_loop, uses, fs);
            // two copies of the body must fit the size up to which pair mode is taken at all (eligible)
            const bool guarded = std::any_of(fs.begin(), fs.end(), [&](const Fuse &f) { return needs_guard(f.b); });
            if (!fs.empty() && (!guarded || 2 * count_stmts(s->body) <= (env.knobs.pair.has_value() ? 400 : 40))) fuse_plan[s] = fs;
            plan_loops(s->body, uses);
            for (const Stmt *ph : ivs) uniform.erase(ph->lhs);
        }
    }
    void plan_fusion() {
        if (!fma2) return;
        const Uses uses = count_uses();
        const std::set<const Value *> keep = uniform;
        plan_loops(code.body, uses);
        uniform = keep;
    }
    static bool needs_guard(const Primary &b) { return b.kind == Primary::Val && b.value->index >= 0; }
    // The loop `w` with fused statements.  The guard -- no lane's addend above 2^102, in either pixel; the lanes of columns past the
    // frame's edge have returned, rows past its end hold the last row's values -- is wave-uniform, and the loop is printed
    // twice under it: today's text under its own names (mm_l<id>) for a wave in which it fails, the fused text under a
    // label number of its own.  Both copies read and leave the same phis, mask and exit copies.
    void fused_loop(const Loop &w, const std::vector<Fuse> &fs, const std::string &id, const std::string &mask) {
        const std::string &ind = w.ind, I1 = ind + "  ";
        std::vector<std::string> addends;
        for (const Fuse &f : fs) {
            if (!needs_guard(f.b)) continue;
            const std::string b = pprim(f.b, Ty::Float);
            if (std::find(addends.begin(), addends.end(), b) == addends.end()) addends.push_back(b);
        }
        auto copy = [&](bool fused, const std::string &l, const std::string &I) {
            Loop c = w;
            c.ind = I;
            if (fused) for (const Fuse &f : fs) { fusing[f.r] = &f; if (!f.keep_d) fused_away.insert(f.d); }
            plan_counted(c, l);
            // (the fast step: each copy tests its own scalar copy of the mask -- one test ahead of the guard, read by both copies, is a
            // truth value that lives across a branch, which this compiler carries in a vector register: v_cndmask_b32, v_cmp_ne_u32)
            if (fast_step && !addends.empty()) out << I << "asm(\"\" : \"+s\"(" << c.a << ".x), \"+s\"(" << c.a << ".y));\n";
            out << I << "while (" << c.a << ".x | " << c.a << ".y) {\n";
            exit_driven_iteration(c, l);
            out << I << "}\n";
            if (fused) for (const Fuse &f : fs) { fusing.erase(f.r); fused_away.erase(f.d); }
        };
        out << ind << "mm_bb " << w.a << " = mm_andb(" << mask << ", " << pbool(w.s->cond.prim) << ");\n";
        if (addends.empty()) { copy(true, "mm_l" + id, ind); return; }
        out << ind << "const bool mm_g" << id << " = ";
        for (size_t i = 0; i < addends.size(); ++i) out << (i ? " && " : "") << "mm_fma2_ok(" << addends[i] << ")";
        out << ";\n" << ind << "if (!mm_g" << id << ") {\n";
        copy(false, "mm_l" + id, I1);
        out << ind << "} else {\n";
        copy(true, "mm_l" + std::to_string(ids++), I1);
        out << ind << "}\n";
    }
    // A `while` under `mask`: runs while either pixel is in it.  The two shapes share everything but the iteration.
    void while_loop(Stmt *s, const std::string &ind, const std::string &mask) {
        const std::string id = std::to_string(ids++);
        Loop w{s, ind, "mm_a" + id, {}, {}, {}};
        uses_outside(code.body, s, w.outside);
        for (int i = 0; i < 4; ++i) w.outside.insert(code.result[i]);
        // (selects freeze the condition too: it is tested again after its pixel has left)
        if (!exit && s->cond.prim.kind == Primary::Val) w.outside.insert(s->cond.prim.value);
        for (Stmt *ph : s->phis)
            if (ph->in_pixel) out << ind << vname(ph->lhs) << " = " << pval_as(ph->rhs.prim, ph->lhs) << ";\n";
        if (exit) {      // exit copies of the phis that are read after the loop: a pixel that never enters it sees the initial value
            int k = 0;
            for (Stmt *ph : s->phis) {
                if (!ph->in_pixel) continue;
                if (w.outside.count(ph->lhs)) w.exit_copy.push_back({ph, w.a + "_e" + std::to_string(k)});
                ++k;      // (numbered like the phis)
            }
            for (const auto &e : w.exit_copy) out << ind << pair_ctype(e.first->lhs) << " " << e.second << " = " << vname(e.first->lhs) << ";\n";
        }
        w.ivs = find_uniform_ivs(s);
        for (const Stmt *ph : w.ivs) {
            uniform.erase(ph->lhs);       // the initial value is printed with the ordinary names
            const std::string init = env.prim(ph->rhs.prim);
            uniform.insert(ph->lhs);
            out << ind << (ph->lhs->var->type == Ty::Float ? "float u" : "int u") << vname(ph->lhs) << " = " << init << ";\n";
        }
        const auto fp = fuse_plan.find(s);
        if (fp != fuse_plan.end()) fused_loop(w, fp->second, id, mask);
        else {
            if (exit) plan_counted(w, "mm_l" + id);
            out << ind << "mm_bb " << w.a << " = mm_andb(" << mask << ", " << pbool(s->cond.prim) << ");\n";
            out << ind << "while (" << w.a << ".x | " << w.a << ".y) {\n";
            if (exit) exit_driven_iteration(w, "mm_l" + id);
            else selecting_iteration(w);
            out << ind << "}\n";
        }
        for (const auto &e : w.exit_copy) out << ind << vname(e.first->lhs) << " = " << e.second << ";\n";      // read through it from here on
        for (const Stmt *ph : w.ivs) uniform.erase(ph->lhs);
    }

    // ---- statements; `mask`: the expression (mm_bb) under which the block runs ----
    void stmts(Block &b, const std::string &ind, const std::string &mask) {
        for (Stmt *s : b) {
            if (!s->in_pixel) continue;
            switch (s->kind) {
                case Stmt::Assign:
                    if (s == split_def) {       // tested at the back edge (exit_driven_iteration): inside the loop it holds
                        out << ind << "const bool u" << vname(s->lhs) << " = " << (split_leave ? "false" : "true") << ";\n";
                        break;
                    }
                    if (uniform.count(s->lhs)) {       // scalar statement, the scalar kernel's own expression
                        const char *ty = bools.count(s->lhs) ? "bool" : s->lhs->var->type == Ty::Float ? "float" : "int";
                        out << ind << "const " << ty << " u" << vname(s->lhs) << " = " << env.rhs(s) << ";\n";
                        break;
                    }
                    if (fused_away.count(s)) break;      // its one reader multiplies by itself
                    if (fusing.count(s)) {
                        const Fuse &f = *fusing.at(s);
                        const std::string t = pprim(f.t, Ty::Float), k = float_literal(f.k) + "f", b = pprim(f.b, Ty::Float);
                        out << ind << vname(s->lhs) << " = mm_pf{__builtin_fmaf(" << t << ".x, " << k << ", " << b << ".x), __builtin_fmaf("
                            << t << ".y, " << k << ", " << b << ".y)};\n";
                        break;
                    }
                    out << ind << vname(s->lhs) << " = " << prhs(s->rhs, s->lhs) << ";\n";
                    break;
                case Stmt::If: {
                    const std::string c = "mm_c" + std::to_string(ids++);
                    out << ind << "const mm_bb " << c << " = " << pbool(s->cond.prim) << ";\n";
                    stmts(s->then_, ind, "mm_andb(" + mask + ", " + c + ")");
                    stmts(s->else_, ind, "mm_andb(" + mask + (exit ? ", mm_xnotb(" : ", mm_notb(") + c + "))");
                    for (Stmt *ph : s->phis)
                        if (ph->in_pixel)
                            out << ind << vname(ph->lhs) << " = mm_sel2(" << c << ", " << pval_as(ph->rhs.prim, ph->lhs) << ", "
                                << pval_as(ph->rhs2.prim, ph->lhs) << ");\n";
                    break;
                }
                case Stmt::While: while_loop(s, ind, mask); break;
                default: break;
            }
        }
    }

    // (this text is part of the kernels' cache keys: it still names the function as it was called when it was written)
    void emit_helpers() override {
        if (exit)      // emitted behind the preludes, not in the device prelude: the other kernels' text, and keys, stay as they were
            out << R"(#define MM_PAIR_EXIT 1
// exit-driven pair loops (hipgen.cpp pair_while_exit).  mm_xnotb: a lane mask's bits outside exec are never read -- selects
// read their own lane's bit, and every mask a branch tests is ANDed with one that lies inside exec -- so NOT needs no re-AND
// and a broadcast no ballot.
MM_DEV mm_bb mm_xnotb(mm_bb a) { return mm_bb{~a.x, ~a.y}; }
MM_DEV mm_bb mm_xbu(bool u) { const unsigned long m = u ? ~0ul : 0ul; return mm_bb{m, m}; }      // a literal truth value, likewise
// a wave-uniform int for the exit copies, moved from its scalar register where it is wanted (as an ordinary operand it
// would pull the loop counter, and the loop's bound test, onto the vector unit)
MM_DEV int mm_s2v(int u) { int r; asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(__builtin_amdgcn_readfirstlane(u))); return r; }
)";
        bool guarded = false;      // (a loop whose addends are all literals is fused as it stands)
        for (const auto &lp : fuse_plan) for (const Fuse &f : lp.second) guarded = guarded || needs_guard(f.b);
        if (guarded)
            out << R"(#define MM_PAIR_FMA2 1
// fused doubling (hipgen_pair.cpp plan_fusion): fl(fl(t * 2^k) + b) is fma(t, 2^k, b) -- the product is exact -- unless the
// product overflows and the exact sum does not, which takes |b| > 2^103.  True when no lane of the wave holds such an
// addend in either pixel (NaN fails the comparison): the loop then runs in its fused copy.
MM_DEV bool mm_fma2_ok(mm_pf b) {
  return __builtin_amdgcn_ballot_w64(!(__builtin_fabsf(b.x) <= 0x1p102f && __builtin_fabsf(b.y) <= 0x1p102f)) == 0ul;
}
)";
        if (fast_step)
            out << R"(#define MM_PAIR_STEP 1
// the fast pair step (hipgen_pair.cpp emit_pixel_loop): a step that lies inside the launch's rows addresses the y table and the
// output as a wave-uniform 64-bit base -- the tile's first row -- plus a 32-bit lane offset that follows mm_p.  The offset is
// formed next to the access, so base and offset go into the instruction's own saddr form: no 64-bit vector arithmetic is left.
MM_DEV mm_pf mm_load_y2(const char *sy, unsigned oy) {      // both rows' y, one 8-byte load (the offset is a multiple of 8)
  typedef float mm_y2v __attribute__((ext_vector_type(2)));
  const mm_y2v y = *(const mm_y2v *)(sy + oy);
  return mm_pf{y.x, y.y};
}
// a frame constant read as a truth value: wave-uniform, so its lane mask is all ones or zero and is made on the scalar unit, once,
// in front of the pixel loop.  Bits outside exec are set: mm_xnotb's argument covers it (selects read their own lane's bit, and
// the mask a loop tests is ANDed with mm_bu(true), which lies inside exec).  (Through a scalar register by name: a select between
// 64-bit constants on a uniform bool is a v_cndmask_b32 pair to this compiler.)
MM_DEV mm_bb mm_xbs(int u) {
  unsigned long m = (unsigned long)(long)__builtin_amdgcn_readfirstlane(u != 0 ? -1 : 0);
  asm("" : "+s"(m));
  return mm_bb{m, m};
}
)";
        emit_store_pair();
    }

    // ---- the result pack of this kernel ----
    // mm_store_pixel packs four channels it knows nothing about, once per pixel.  Here the channels are known: which of them
    // are the same SSA value (a grey result is one value three times) and which are literals (alpha = 1 of every filter that
    // does not compute one).  mm_store_pair, emitted for this kernel alone, stores both pixels of a step: on the RGBA8 path
    // (bpp 4, no floatmap) every distinct value is clamped and converted once, all of them inside one round-toward-zero
    // window, a literal channel is its byte -- floor(255 clamp(c)), what mm_pack_rgba8 computes -- and v_perm_b32 puts byte 0
    // of each converted value where its channels are.  Every other output format goes through mm_store_pixel as before.
    struct Pack {
        std::vector<const Value *> vals;      // the distinct values that are converted
        int src[4];                           // per channel: index into vals, or -1: a literal
        float lit[4];
    };
    static bool literal_of(const Value *v, float &f, int depth = 0) {
        if (!v || depth > 8) return false;
        if (v->index < 0) { f = 0; return true; }      // uninitialised: reads as 0
        const Stmt *d = v->def;
        if (!d || d->kind != Stmt::Assign || d->lhs != v || d->rhs.kind != Rhs::Prim) return false;
        const Primary &p = d->rhs.prim;
        if (p.kind == Primary::IntConst) { f = (float)p.i; return true; }
        if (p.kind == Primary::FloatConst) { f = p.f; return v->var->type == Ty::Float && f == f; }
        return p.kind == Primary::Val && p.value->var->type == v->var->type && literal_of(p.value, f, depth + 1);
    }
    bool plan_pack(Pack &pk) const {
        if (!pack) return false;
        for (int i = 0; i < 4; ++i) {
            const Value *v = code.result[i];
            pk.src[i] = -1;
            if (literal_of(v, pk.lit[i])) continue;
            const auto it = std::find(pk.vals.begin(), pk.vals.end(), v);
            pk.src[i] = (int)(it - pk.vals.begin());
            if (it == pk.vals.end()) pk.vals.push_back(v);
        }
        return !pk.vals.empty();
    }
    void emit_store_pair() {
        Pack pk;
        if (!plan_pack(pk)) return;
        const int n = (int)pk.vals.size();
        unsigned k = 0;                       // the literal channels' bytes, in place
        for (int i = 0; i < 4; ++i)
            if (pk.src[i] < 0) {
                const float c = pk.lit[i] < 0.0f ? 0.0f : pk.lit[i] > 1.0f ? 1.0f : pk.lit[i];
                k |= (unsigned)(255.0 * (double)c) << (8 * i);
            }
        // v_perm_b32 selectors: 0x00 / 0x04: byte 0 of the second / first operand, 0x0c: a zero byte
        auto sel = [&](int second, int first) {
            unsigned s = 0;
            for (int i = 0; i < 4; ++i) s |= (pk.src[i] == second && second >= 0 ? 0x00u : pk.src[i] == first && first >= 0 ? 0x04u : 0x0cu) << (8 * i);
            return s;
        };
        auto hex = [](unsigned v) { char b[16]; snprintf(b, sizeof b, "0x%08xu", v); return std::string(b); };
        auto word = [&](const char *px) {
            auto u = [&](int j) { return std::string("u") + px + std::to_string(j); };
            if (n == 1) {      // the literals' bytes come from the constant word: its byte i for channel i
                unsigned s1 = 0;
                for (int i = 0; i < 4; ++i) s1 |= (pk.src[i] == 0 ? 0x04u : (unsigned)i) << (8 * i);
                return "__builtin_amdgcn_perm(" + u(0) + ", " + hex(k) + ", " + hex(s1) + ")";
            }
            std::string w = "__builtin_amdgcn_perm(" + u(1) + ", " + u(0) + ", " + hex(sel(0, 1)) + ")";
            if (n > 2) w += " | __builtin_amdgcn_perm(" + (n > 3 ? u(3) : u(2)) + ", " + u(2) + ", " + hex(sel(2, n > 3 ? 3 : -1)) + ")";
            return k ? w + " | " + hex(k) : w;
        };
        // clamp, convert inside one round-toward-zero window: ua<j>, ub<j> hold the bytes of value j
        auto convert = [&](const char *I) {
            out << I;
            for (int j = 0; j < n; ++j) out << " a" << j << " = mm_clamp01(a" << j << "); b" << j << " = mm_clamp01(b" << j << ");";
            out << "\n" << I << " unsigned";
            for (int j = 0; j < n; ++j) out << (j ? ", " : " ") << "ua" << j << ", ub" << j;
            out << ";\n" << I << " asm volatile(\"s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\\n\\t\"\n";
            for (int j = 0; j < 2 * n; ++j) out << I << "              \"v_fma_f32 %" << j << ", %" << 2 * n + j << ", %" << 4 * n << ", %" << 4 * n + 1 << "\\n\\t\"\n";
            out << I << "              \"s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\"\n" << I << "              :";
            for (int j = 0; j < n; ++j) out << (j ? ", " : " ") << "\"=&v\"(ua" << j << "), \"=&v\"(ub" << j << ")";
            out << "\n" << I << "              :";
            for (int j = 0; j < n; ++j) out << " \"v\"(a" << j << "), \"v\"(b" << j << "),";
            out << " \"s\"(255.0f), \"v\"(8388608.0f));\n";
        };
        out << "// this kernel's result pack (hipgen_pair.cpp emit_store_pair): both pixels of a step, " << n << " distinct value" << (n > 1 ? "s" : "")
            << " per pixel, literal bytes " << hex(k) << "\n"
            << "MM_DEV void mm_store_pair(const mm_args &A, int row_a, int row_b, int col";
        for (int j = 0; j < n; ++j) out << ", float a" << j << ", float b" << j;
        out << ") {\n  if (__builtin_expect(!A.floatmap && A.output_bpp == 4, 1)) {\n";
        convert("   ");
        out << "    MM_STORE_U32((unsigned *)((unsigned char *)A.out + (long)row_a * A.row_stride + (long)col * 4), " << word("a") << ");\n"
            << "    MM_STORE_U32((unsigned *)((unsigned char *)A.out + (long)row_b * A.row_stride + (long)col * 4), " << word("b") << ");\n"
            << "    return;\n  }\n  mm_tup<4> ra, rb;\n";
        for (int i = 0; i < 4; ++i) {
            if (pk.src[i] < 0) out << "  ra.v[" << i << "] = rb.v[" << i << "] = " << float_literal(pk.lit[i]) << "f;\n";
            else out << "  ra.v[" << i << "] = a" << pk.src[i] << "; rb.v[" << i << "] = b" << pk.src[i] << ";\n";
        }
        out << "  mm_store_pixel(A, row_a, col, ra);\n  mm_store_pixel(A, row_b, col, rb);\n}\n";
        if (!fast_step) return;
        out << "// the same words from a fast step (mm_load_y2, above): `so` the step's first output row, oa / ob this lane's offsets in its two rows\n"
            << "MM_DEV void mm_store_step(unsigned char *so, unsigned oa, unsigned ob";
        for (int j = 0; j < n; ++j) out << ", float a" << j << ", float b" << j;
        out << ") {\n";
        convert(" ");
        out << "  MM_STORE_U32((unsigned *)(so + oa), " << word("a") << ");\n"
            << "  MM_STORE_U32((unsigned *)(so + ob), " << word("b") << ");\n}\n";
    }
    // two pixels (rows mm_p and mm_p + 1 of this work-item's column) in lockstep
    //
    // The fast step (MMHIP_PAIR_STEP unset or 1; 0: the step as it was, byte for byte).  A workgroup's tile is MM_TILE_W columns by
    // MM_TILE_H * A.ppt rows, a step covers 2 * MM_TILE_H consecutive rows of it, and a work-item's rows are 2 * (threadIdx.x /
    // MM_TILE_W) and the next one from the step's first row.  So a lane's byte offsets from the tile's first row -- in the output and
    // in the y table -- are known in front of the pixel loop, that row is wave-uniform (two 64-bit bases, made once), and a step
    // adds its distance from it, a multiple of mm_p, to the 32-bit offsets: one scalar multiply and three 32-bit vector adds.  The
    // step as it was computes both rows, clamps them to the launch's last row and forms three 64-bit addresses per lane (two of
    // them 64-bit multiply-adds), every step.  It is still there, unchanged, for a step whose last row lies past the launch's
    // rows (the clamp is needed there) and for every launch the fast step is not for: another output format than RGBA8
    // (mm_store_pair's own branch), a lane offset that does not fit 32 bits, a y table or a tile height that would misalign the
    // 8-byte load.  All of that is decided once, at kernel entry (mm_fast), and folded into mm_pin, the steps of this tile that lie
    // inside the launch's rows: the test per step is mm_p < mm_pin, wave-uniform.  No address is truncated: the bases are 64-bit,
    // and a frame too large for 32-bit lane offsets renders by the other step.  The loops are printed once; only what stands in
    // front of them and behind them is chosen per step.  Nothing is advanced per step and the test is written as one-sided ifs on
    // copies of mm_pin because scalar instructions are what this kernel has least room for (a CU's scalar unit serves four SIMDs):
    // with both bases advanced and one truth value for the test the step was slower than the one it replaces.
    void emit_pixel_loop(const std::string &I) override {
        Pack pk;
        const bool packed = plan_pack(pk);
        if (fast_step) {      // (only with a pack: make_pair_mode)
            // the loop's text first: it says which frame constants it reads as truth values (pbool)
            std::ostringstream body;
            std::streambuf *const own = out.rdbuf(body.rdbuf());
            emit_steps(I, pk, packed);
            out.rdbuf(own);
            // what depends on the lane and the column alone; the first row `sr` the steps start from and what follows from it
            auto lane_head = [](const std::string &I, const char *offsets) {
                return I + "// the fast step (hipgen_pair.cpp emit_pixel_loop): decided once; this lane's offsets from the tile's first row, that row's wave-uniform bases\n" +
                       I + "const bool mm_fast = !A.floatmap && A.output_bpp == 4 && A.row_stride >= 0 && ((MM_TILE_H * A.ppt) & 1) == 0 && ((unsigned long)A.ytab & 7ul) == 0ul &&\n" +
                       I + "                     (long)(MM_TILE_H * (A.ppt + 1) - 1) * A.row_stride + (long)A.region_width * 4 <= 0xffffffffl;\n" +
                       I + "const unsigned mm_tr = threadIdx.x / MM_TILE_W;\n" +
                       I + offsets + " mm_oa = (unsigned)col * 4u + 2u * mm_tr * (unsigned)A.row_stride, mm_ob = mm_oa + (unsigned)A.row_stride, mm_oy = 8u * mm_tr;\n" +
                       I + "const unsigned mm_ss = (unsigned)(MM_TILE_H * A.row_stride);      // mm_p counts rows MM_TILE_H apart\n";
            };
            auto row_head = [](const std::string &I, const std::string &sr) {
                return I + "const int mm_sr = __builtin_amdgcn_readfirstlane(" + sr + ");\n" +
                       I + "unsigned char *const mm_so = (unsigned char *)A.out + (long)mm_sr * A.row_stride;\n" +
                       I + "const char *const mm_sy = (const char *)(A.ytab + mm_sr);\n" +
                       I + "// the steps, in mm_p, that lie inside the launch's rows (none: not a launch for the fast step): one scalar compare per step\n" +
                       I + "const int mm_pin = mm_fast ? (A.num_rows - mm_sr) / (2 * MM_TILE_H) * 2 : 0;\n";
            };
            auto pin_copies = [](const std::string &I) {
                return I + "// (a copy per test: one truth value read in several places would live across branches, which this compiler keeps as a lane\n" +
                       I + "// mask -- s_cselect_b64, s_and_b64 with exec, a branch on vcc -- and an if / else on it goes through a flag block; four one-sided\n" +
                       I + "// tests of scalars the compiler takes for unrelated are s_cmp and a branch on scc each)\n" +
                       I + "int mm_pin_a = mm_pin, mm_pin_b = mm_pin, mm_pin_c = mm_pin;\n" +
                       I + "asm(\"\" : \"+s\"(mm_pin_a), \"+s\"(mm_pin_b), \"+s\"(mm_pin_c));\n";
            };
            std::string masks;
            for (size_t k = 0; k < entry_masks.size(); ++k)
                masks += I + "const mm_bb mm_ub" + std::to_string(k) + " = mm_xbs(" + entry_masks[k] + ");\n";
            const std::string steps = body.str();
            const std::string tile = lane_head(I, "const unsigned") + row_head(I, "tile_y * (MM_TILE_H * A.ppt)") + pin_copies(I) + masks + steps;      // consecutive steps
            if (!spread) {
                out << tile;
                return;
            }
            // Spread steps (MMHIP_PAIR_SPREAD unset or 1; 0: the text as it was), the single-frame kernel only.  A workgroup's cost
            // follows where its tile lies -- inside the set every pixel runs to the iteration limit -- and only a few workgroups
            // pass through a wave slot per launch, so the heavy ones that were handed out late finish alone while the other slots
            // stand empty.  The workgroup keeps its columns and its A.ppt / 2 steps, but the steps are no longer consecutive:
            // step k (a segment) starts mm_nty steps behind step k - 1, mm_nty the launch's tile rows, so every workgroup takes its
            // rows from all over the frame's height and costs about what its column costs.  The segments of all workgroups tile
            // the launch's step rows exactly once ((k, tile_y) -> k * mm_nty + tile_y is one to one onto [0, mm_nty * A.ppt / 2));
            // one that starts at or past the last row has nothing to do, and neither has any later one.  The step loop below is
            // the text as it was with one trip per segment (mm_p stays 0); a clip launch has workgroups enough and keeps its text.
            //   What a segment needs -- its first row, the two bases, mm_pin -- is computed for the first one by the statements the
            // text had and advanced from there by scalar additions: recomputed per segment (a 64-bit multiply, a division, the
            // select on mm_fast) the step had 40 scalar instructions where the consecutive one has 15, and rendered 4 % slower.
            //   The step as it was counts its rows from `row0`: each of its two blocks gets one of its own, the segment's first row
            // plus the lane's, behind an empty asm -- a segment's rows no longer follow mm_p, and the compiler would compute them,
            // clamps and all, in front of the branch for every step (five vector instructions for blocks that run once per frame).
            const std::string J = I + "  ", E = I + "    ";
            auto replace_all = [](std::string s, const std::string &was, const std::string &is) {
                for (size_t at = s.find(was); at != std::string::npos; at = s.find(was, at + is.size())) s.replace(at, was.size(), is);
                return s;
            };
            const std::string rows_was = E + "const int rl_a = row0 + ";
            const std::string seg = replace_all(replace_all(steps, "for (; mm_p < A.ppt; mm_p += 2) {\n", "for (mm_p = 0; mm_p < 2; mm_p += 2) {      // one step per segment\n"), rows_was,
                                                E + "int row0 = mm_sr;      // the segment's first row, not the tile's\n" +
                                                E + "asm volatile(\"\" : \"+s\"(row0));\n" +
                                                E + "row0 += (int)(threadIdx.x / MM_TILE_W);\n" + rows_was);
            std::string body_in;
            for (size_t b = 0, e; b < seg.size(); b = e + 1) {      // one level deeper (preprocessor lines stay where they are)
                e = seg.find('\n', b);
                if (e == std::string::npos) e = seg.size() - 1;
                body_in += (seg[b] == '#' || seg[b] == '\n' ? "" : "  ") + seg.substr(b, e + 1 - b);
            }
            env.emit_both(lane_head(I, "unsigned") + masks +
                              I + "// spread steps (hipgen_pair.cpp emit_pixel_loop): segment k of this workgroup is step k * mm_nty + tile_y of the launch's rows\n" +
                              I + "const int mm_nty = (A.tiles_magic ? (int)__umulhi((unsigned)(nwg - 1), A.tiles_magic) : (nwg - 1) / tiles_x) + 1;      // the launch's tile rows\n" +
                              I + "// the first segment: its first row, the bases there, the whole steps (times two) from that row to the launch's last\n" +
                              row_head(I, "tile_y * (2 * MM_TILE_H)") +
                              I + "// from segment to segment all of them move by mm_nty steps -- one scalar addition each, nothing is multiplied or divided per\n" +
                              I + "// step -- up to the workgroup's last segment or the launch's last row: a segment that starts at or past it has nothing to do\n" +
                              I + "const int mm_ds = mm_nty * (2 * MM_TILE_H), mm_last = mm_sr + (A.ppt >> 1) * mm_ds, mm_end = mm_last < A.num_rows ? mm_last : A.num_rows;\n" +
                              I + "const long mm_dso = (long)mm_ds * A.row_stride;\n" +
                              I + "int mm_srk = mm_sr, mm_pink = mm_pin;\n" +
                              I + "unsigned char *mm_sok = mm_so;\n" +
                              I + "const char *mm_syk = mm_sy;\n" +
                              "#pragma nounroll\n" +
                              I + "for (; mm_srk < mm_end; mm_srk += mm_ds, mm_sok += mm_dso, mm_syk += 4 * mm_ds, mm_pink -= 2 * mm_nty) {\n" +
                              J + "const int mm_sr = mm_srk, mm_pin = mm_pink;      // this segment's, under the names the step knows\n" +
                              J + "unsigned char *const mm_so = mm_sok;\n" +
                              J + "const char *const mm_sy = mm_syk;\n" +
                              pin_copies(J) +
                              J + "// (the lane offsets no longer change from step to step: left to itself the compiler adds them to the frame's base once, as\n" +
                              J + "// 64-bit vector addresses, and adds the segment's distance to those per step -- the saddr form, a scalar base and these\n" +
                              J + "// 32-bit offsets, needs no vector instruction at all)\n" +
                              J + "asm volatile(\"\" : \"+v\"(mm_oa), \"+v\"(mm_ob), \"+v\"(mm_oy));\n" +
                              body_in + I + "}\n",
                          tile);
            return;
        }
        emit_steps(I, pk, packed);
    }
    void emit_steps(const std::string &I, const Pack &pk, bool packed) {
        const std::string E = fast_step ? I + "  " : I;      // the step as it was: inside an else
        out << "#pragma unroll 1\n" << I << "for (; mm_p < A.ppt; mm_p += 2) {\n";
        if (fast_step)
            out << I << "  const bool mm_in = mm_p < mm_pin;      // wave-uniform: the fast step is for this launch and the whole step lies inside its rows\n"
                << I << "  mm_pf mm_y2;\n"
                << I << "  if (__builtin_expect(mm_in, 1)) mm_y2 = mm_load_y2(mm_sy, mm_oy + (unsigned)mm_p * (4u * MM_TILE_H));\n"
                << I << "  if (__builtin_expect(mm_p >= mm_pin_a, 0)) {      // (!mm_in) the step as it was\n";
        out << E << "  // vertically adjacent pixels: they mostly take the same path (a wave covers 16 x 8 pixels per step)\n"
            << E << "  const int rl_a = row0 + (int)(threadIdx.x / MM_TILE_W) + mm_p * MM_TILE_H, rl_b = rl_a + 1;\n"
            << E << "  const int row_a = rl_a < A.num_rows ? rl_a : A.num_rows - 1, row_b = rl_b < A.num_rows ? rl_b : A.num_rows - 1;\n"
            << E << (fast_step ? "  mm_y2 = mm_pf{A.ytab[row_a], A.ytab[row_b]};" : "  const mm_pf mm_y2 = {A.ytab[row_a], A.ytab[row_b]};") << "    // CALC_VIRTUAL_Y per row, by the prologue\n";
        if (fast_step) out << I << "  }\n";
        std::set<Value *> seen;
        for (Value *v : env.pix_defs)
            if (v->index >= 0 && seen.insert(v).second) out << I << "  " << pair_ctype(v) << " " << vname(v) << ";\n";
        stmts(code.body, I + "  ", "mm_bu(true)");
        if (packed) {
            std::string vals;
            for (const Value *v : pk.vals) {
                const std::string e = pprim(Primary::V(const_cast<Value *>(v)), Ty::Float);
                vals += ", " + e + ".x, " + e + ".y";
            }
            if (fast_step)
                out << I << "  if (__builtin_expect(mm_p < mm_pin_b, 1)) {      // (mm_in)\n"
                    << I << "    const unsigned mm_sp = (unsigned)mm_p * mm_ss;\n"
                    << I << "    mm_store_step(mm_so, mm_oa + mm_sp, mm_ob + mm_sp" << vals << ");\n"
                    << I << "  }\n"
                    << I << "  if (__builtin_expect(mm_p >= mm_pin_c, 0)) {      // (!mm_in) the step as it was\n"
                    << E << "  const int rl_a = row0 + (int)(threadIdx.x / MM_TILE_W) + mm_p * MM_TILE_H, rl_b = rl_a + 1;\n"
                    << E << "  const int row_a = rl_a < A.num_rows ? rl_a : A.num_rows - 1, row_b = rl_b < A.num_rows ? rl_b : A.num_rows - 1;\n";
            out << E << "  // a row past the end was evaluated as the last row: storing it there again writes the same bytes\n"
                << E << "  mm_store_pair(A, row_a, row_b, col" << vals << ");\n";
            if (fast_step)
                out << I << "  }\n";
            out << I << "}\n";
            return;
        }
        out << I << "  mm_tup<4> mm_ra, mm_rb;\n";
        for (int i = 0; i < 4; ++i) {
            const std::string v = pprim(Primary::V(code.result[i]), Ty::Float);
            out << I << "  mm_ra.v[" << i << "] = " << v << ".x; mm_rb.v[" << i << "] = " << v << ".y;\n";
        }
        out << I << "  // a row past the end was evaluated as the last row: storing it there again writes the same bytes\n"
            << I << "  mm_store_pixel(A, row_a, col, mm_ra);\n"
            << I << "  mm_store_pixel(A, row_b, col, mm_rb);\n" << I << "}\n";
    }
};

}  // namespace

std::unique_ptr<PairMode> make_pair_mode(const PairEnv &env) {
    std::unique_ptr<PairGen> g(new PairGen(env));
    if (!g->eligible()) return nullptr;
    g->infer_bools();
    g->plan_fusion();
    PairGen::Pack pk;
    // (with a fused loop only: a kernel in which nothing is fused has one text under either value of MMHIP_PAIR_FMA2, and
    // MMHIP_PAIR_FMA2=0 is one of the switches that keep their text)
    g->fast_step = g->step && !g->fuse_plan.empty() && g->plan_pack(pk);
    g->spread = g->fast_step && env.knobs.pair_spread.value_or(1);
    return g;
}

}  // namespace hipgen
}  // namespace mm
