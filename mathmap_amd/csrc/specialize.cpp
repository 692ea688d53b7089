// User-value specialisation: constant propagation over the structured SSA.
//
// When a filter is invoked, its scalar user values are known.  The specialising JIT lowers
// the filter with those values as literals and then applies, to what are now literal
// constants, exactly the folds the reference's own optimiser applies to literals
// (constant folding through the op macros, compiler.c:3383-3458, and simplify_ops,
// compiler.c:3460-3535: x+0, 0+x, x-0 -> x; x*1, 1*x, x/1 -> x; x*0, 0*x -> 0), followed by
// dead-branch removal (compiler.c:3537-3700).  Constants are propagated *optimistically*
// through loop phis (sparse-conditional-constant style lattice: Top > Const > Bottom), so a
// component that starts at 0 and is only ever multiplied/added with zeros (e.g. the j,k parts
// of the quaternion Mandelbrot for cj = ck = pj = pk = 0) disappears from the kernel.
//
// Like the reference's literal folds, x*0 -> 0 ignores NaN/Inf in x; the generic
// (unspecialised) kernel remains the default and the reference for parity tests.
#include <cmath>
#include <cstring>
#include <functional>
#include <map>

#include "passes.h"

namespace mm {

namespace {

struct Lat {
    enum K { Top, Const, Bottom } k = Top;
    Primary c;
};

bool same_const(const Primary &a, const Primary &b) {
    if (a.kind != b.kind) return false;
    if (a.kind == Primary::IntConst) return a.i == b.i;
    if (a.kind == Primary::FloatConst) return std::memcmp(&a.f, &b.f, 4) == 0;
    return false;
}

bool is_zero(const Primary &p) {
    return (p.kind == Primary::IntConst && p.i == 0) || (p.kind == Primary::FloatConst && p.f == 0.0f);
}
bool is_one(const Primary &p) {
    return (p.kind == Primary::IntConst && p.i == 1) || (p.kind == Primary::FloatConst && p.f == 1.0f);
}
double as_double(const Primary &p) { return p.kind == Primary::IntConst ? (double)p.i : (double)p.f; }

// C assignment conversion of a constant to the type of the variable it is stored in
bool convert_to(Ty t, Primary &p) {
    const bool of_variable = p.of_variable;
    if (t == Ty::Int) {
        if (p.kind == Primary::FloatConst) {
            if (!(std::fabs(p.f) < 2e9f)) return false;
            p = Primary::I((int)p.f);
            p.of_variable = of_variable;
        }
        return p.kind == Primary::IntConst;
    }
    if (t == Ty::Float) {
        if (p.kind == Primary::IntConst) {
            p = Primary::F((float)p.i);
            p.of_variable = of_variable;
        }
        return p.kind == Primary::FloatConst;
    }
    return false;
}

bool both_int(const Primary &a, const Primary &b) { return a.kind == Primary::IntConst && b.kind == Primary::IntConst; }

// folds an operator on constants with the C semantics of its macro (opmacros.h)
bool fold_values(const OpInfo *op, const std::vector<Primary> &a, Primary &out) {
    const char *n = op->cname;
    auto bin = [&](auto fi, auto fd) {
        if (both_int(a[0], a[1])) out = Primary::I(fi(a[0].i, a[1].i));
        else out = Primary::F((float)fd(as_double(a[0]), as_double(a[1])));   // double op, one rounding (innocuous for + - *)
        return true;
    };
    if (!strcmp(n, "ADD")) return bin([](int x, int y) { return (int)((unsigned)x + (unsigned)y); }, [](double x, double y) { return x + y; });
    if (!strcmp(n, "SUB")) return bin([](int x, int y) { return (int)((unsigned)x - (unsigned)y); }, [](double x, double y) { return x - y; });
    if (!strcmp(n, "MUL")) return bin([](int x, int y) { return (int)((unsigned)x * (unsigned)y); }, [](double x, double y) { return x * y; });
    if (!strcmp(n, "NEG")) {
        out = a[0].kind == Primary::IntConst ? Primary::I((int)(0u - (unsigned)a[0].i)) : Primary::F(-a[0].f);
        return true;
    }
    if (!strcmp(n, "DIV")) { out = Primary::F((float)as_double(a[0]) / (float)as_double(a[1])); return true; }
    auto cmp = [&](auto f) { out = Primary::I(both_int(a[0], a[1]) ? f((double)a[0].i, (double)a[1].i) : f(as_double(a[0]), as_double(a[1]))); return true; };
    if (!strcmp(n, "EQ")) return cmp([](double x, double y) { return x == y ? 1 : 0; });
    if (!strcmp(n, "LESS")) return cmp([](double x, double y) { return x < y ? 1 : 0; });
    if (!strcmp(n, "LEQ")) return cmp([](double x, double y) { return x <= y ? 1 : 0; });
    if (!strcmp(n, "NOT") && a[0].kind == Primary::IntConst) { out = Primary::I(!a[0].i); return true; }
    if (!strcmp(n, "MIN") || !strcmp(n, "MAX")) {
        bool pick_first = !strcmp(n, "MIN") ? as_double(a[0]) < as_double(a[1]) : !(as_double(a[0]) < as_double(a[1]));
        const Primary &p = pick_first ? a[0] : a[1];
        out = both_int(a[0], a[1]) ? p : Primary::F((float)as_double(p));
        return true;
    }
    if (!strcmp(n, "INT2FLOAT") && a[0].kind == Primary::IntConst) { out = Primary::F((float)a[0].i); return true; }
    return false;   // libm and everything else stays in the kernel / prologue
}

// fold_values, and the result is the content of a variable where an operand is (Primary::of_variable)
bool fold_impl(const OpInfo *op, const std::vector<Primary> &a, Primary &out) {
    if (!fold_values(op, a, out)) return false;
    out.of_variable = false;
    for (const Primary &p : a) out.of_variable |= p.of_variable;
    return true;
}

struct Sccp {
    static bool fold(const OpInfo *op, const std::vector<Primary> &a, Primary &out) { return fold_impl(op, a, out); }

    FilterCode &code;
    std::map<const Value *, Lat> lat;
    bool changed = false;

    explicit Sccp(FilterCode &c) : code(c) {}

    Lat of(const Primary &p) {
        Lat l;
        if (p.kind == Primary::IntConst || p.kind == Primary::FloatConst) { l.k = Lat::Const; l.c = p; return l; }
        if (p.kind != Primary::Val) { l.k = Lat::Bottom; return l; }
        const Value *v = p.value;
        if (v->index < 0) {   // uninitialised reads as 0
            if (v->var->type == Ty::Int) { l.k = Lat::Const; l.c = Primary::I(0); return l; }
            if (v->var->type == Ty::Float) { l.k = Lat::Const; l.c = Primary::F(0.0f); return l; }
            l.k = Lat::Bottom;
            return l;
        }
        auto it = lat.find(v);
        return it == lat.end() ? Lat() : it->second;
    }

    Lat eval(const Rhs &r, const CompVar *lhs) {
        Lat l;
        switch (r.kind) {
            case Rhs::Prim: l = of(r.prim); break;
            case Rhs::Op: {
                std::vector<Lat> as;
                bool any_top = false, all_const = true;
                for (const Primary &p : r.args) {
                    as.push_back(of(p));
                    any_top |= as.back().k == Lat::Top;
                    all_const &= as.back().k == Lat::Const;
                }
                const char *n = r.op->cname;
                if (!strcmp(n, "MUL") && ((as[0].k == Lat::Const && is_zero(as[0].c)) || (as[1].k == Lat::Const && is_zero(as[1].c)))) {
                    l.k = Lat::Const;
                    l.c = Primary::I(0);
                    break;
                }
                if (any_top) { l.k = Lat::Top; return l; }
                if (all_const && r.op->pure) {
                    std::vector<Primary> cs;
                    for (Lat &x : as) cs.push_back(x.c);
                    Primary out;
                    if (fold(r.op, cs, out)) { l.k = Lat::Const; l.c = out; break; }
                }
                l.k = Lat::Bottom;
                break;
            }
            default: l.k = Lat::Bottom;
        }
        if (l.k == Lat::Const && !convert_to(lhs->type, l.c)) l.k = Lat::Bottom;
        return l;
    }

    static Lat meet(const Lat &a, const Lat &b) {
        if (a.k == Lat::Top) return b;
        if (b.k == Lat::Top) return a;
        if (a.k == Lat::Const && b.k == Lat::Const && same_const(a.c, b.c)) return a;
        Lat l;
        l.k = Lat::Bottom;
        return l;
    }

    void set(const Value *v, const Lat &n) {
        Lat &cur = lat[v];
        Lat m = meet(cur, n);          // monotone descent
        if (cur.k == Lat::Top && n.k == Lat::Top) return;
        if (m.k != cur.k || (m.k == Lat::Const && !same_const(m.c, cur.c))) { cur = m; changed = true; }
    }

    void walk(Block &b) {
        for (Stmt *s : b) {
            switch (s->kind) {
                case Stmt::Assign: set(s->lhs, eval(s->rhs, s->lhs->var)); break;
                case Stmt::If:
                    walk(s->then_);
                    walk(s->else_);
                    for (Stmt *p : s->phis) set(p->lhs, meet(eval(p->rhs, p->lhs->var), eval(p->rhs2, p->lhs->var)));
                    break;
                case Stmt::While:
                    for (Stmt *p : s->phis) set(p->lhs, meet(eval(p->rhs, p->lhs->var), eval(p->rhs2, p->lhs->var)));
                    walk(s->body);
                    for (Stmt *p : s->phis) set(p->lhs, meet(eval(p->rhs, p->lhs->var), eval(p->rhs2, p->lhs->var)));
                    break;
                default: break;
            }
        }
    }

    void run() {
        do {
            changed = false;
            walk(code.body);
        } while (changed);
    }

    // ---- rewriting ------------------------------------------------------------------------
    void subst(Primary &p) {
        if (p.kind != Primary::Val || p.value->index < 0) return;
        auto it = lat.find(p.value);
        if (it != lat.end() && it->second.k == Lat::Const) p = it->second.c;
    }
    void subst(Rhs &r) {
        if (r.kind == Rhs::Prim) subst(r.prim);
        for (Primary &p : r.args) subst(p);
    }

    // simplify_ops identities on the remaining operators
    static void simplify(Rhs &r) {
        if (r.kind != Rhs::Op) return;
        const char *n = r.op->cname;
        auto is_c = [&](int i) { return r.args[i].is_const(); };
        if (!strcmp(n, "ADD")) {
            if (is_c(0) && is_zero(r.args[0])) r = Rhs::P(r.args[1]);
            else if (is_c(1) && is_zero(r.args[1])) r = Rhs::P(r.args[0]);
        } else if (!strcmp(n, "SUB")) {
            if (is_c(1) && is_zero(r.args[1])) r = Rhs::P(r.args[0]);
        } else if (!strcmp(n, "MUL")) {
            if (is_c(0) && is_one(r.args[0])) r = Rhs::P(r.args[1]);
            else if (is_c(1) && is_one(r.args[1])) r = Rhs::P(r.args[0]);
        } else if (!strcmp(n, "DIV")) {
            if (is_c(1) && is_one(r.args[1]) && r.args[0].type() == Ty::Float) r = Rhs::P(r.args[0]);
        }
    }

    static bool truthy(const Primary &p, bool *known) {
        *known = p.kind == Primary::IntConst || p.kind == Primary::FloatConst;
        return p.kind == Primary::IntConst ? p.i != 0 : p.f != 0.0f;
    }

    void rewrite(Block &b) {
        Block out;
        for (Stmt *s : b) {
            switch (s->kind) {
                case Stmt::Assign: {
                    auto it = lat.find(s->lhs);
                    if (it != lat.end() && it->second.k == Lat::Const) s->rhs = Rhs::P(it->second.c);
                    else { subst(s->rhs); simplify(s->rhs); }
                    out.push_back(s);
                    break;
                }
                case Stmt::If: {
                    subst(s->cond);
                    rewrite(s->then_);
                    rewrite(s->else_);
                    for (Stmt *p : s->phis) { subst(p->rhs); subst(p->rhs2); }
                    bool known = false;
                    bool t = s->cond.kind == Rhs::Prim ? truthy(s->cond.prim, &known) : false;
                    if (known) {   // dead branch: splice the live one, phis become plain copies
                        Block &live = t ? s->then_ : s->else_;
                        for (Stmt *x : live) { x->parent = s->parent; out.push_back(x); }
                        for (Stmt *p : s->phis) {
                            Stmt *a = code.new_stmt(Stmt::Assign);
                            a->lhs = p->lhs;
                            a->lhs->def = a;
                            a->rhs = t ? p->rhs : p->rhs2;
                            a->parent = s->parent;
                            out.push_back(a);
                        }
                    } else
                        out.push_back(s);
                    break;
                }
                case Stmt::While: {
                    for (Stmt *p : s->phis) { subst(p->rhs); subst(p->rhs2); }
                    // a loop whose condition is the constant 0 never runs
                    bool known = false, t = true;
                    if (s->cond.kind == Rhs::Prim && s->cond.prim.kind == Primary::Val) {
                        auto it = lat.find(s->cond.prim.value);
                        if (it != lat.end() && it->second.k == Lat::Const) t = truthy(it->second.c, &known);
                    }
                    if (known && !t) {
                        for (Stmt *p : s->phis) {
                            Stmt *a = code.new_stmt(Stmt::Assign);
                            a->lhs = p->lhs;
                            a->lhs->def = a;
                            a->rhs = p->rhs;
                            a->parent = s->parent;
                            out.push_back(a);
                        }
                        break;
                    }
                    subst(s->cond);
                    rewrite(s->body);
                    // phis proven constant turn into assignments in front of the loop
                    Block keep;
                    for (Stmt *p : s->phis) {
                        auto it = lat.find(p->lhs);
                        if (it != lat.end() && it->second.k == Lat::Const) {
                            Stmt *a = code.new_stmt(Stmt::Assign);
                            a->lhs = p->lhs;
                            a->lhs->def = a;
                            a->rhs = Rhs::P(it->second.c);
                            a->parent = s->parent;
                            out.push_back(a);
                        } else
                            keep.push_back(p);
                    }
                    s->phis.swap(keep);
                    out.push_back(s);
                    break;
                }
                default: break;
            }
        }
        b.swap(out);
    }
};

}  // namespace

// Runs constant propagation + simplification + dead-branch removal to a fixpoint.
void specialize_constants(FilterCode &code) {
    propagate_types(code);
    for (int round = 0; round < 8; ++round) {
        Sccp s(code);
        s.run();
        s.rewrite(code.body);
        for (int i = 0; i < 4; ++i) {
            // results must stay values: materialise a constant result
            auto it = s.lat.find(code.result[i]);
            (void)it;
        }
        bool c = copy_propagate(code);
        c |= eliminate_dead_code(code);
        if (!c && round > 0) break;
    }
}

// ---------------------------------------------------------------------------
// Peeling a first trip that folds: `while (c) B` becomes `B0; while (c) B`
// ---------------------------------------------------------------------------
// A specialised loop often enters with literals in its phis (Mandelbrot: c = 0, iter = 0).  The phis hide them from the
// constant propagation above -- the meet of the initial and the next value is Bottom -- so the first trip computes
// `0 * 0 + p` and `0 < 31` for every pixel.  Where the entry condition, evaluated on the phis' initial values, is
// the literal true, the first trip is copied in front of the loop with those values substituted (B0), and the phis start
// from what B0 leaves.  In B0 only folds that are exact for every input are made: an operator all of whose operands are
// literals, through fold_impl; sqrt of a literal whose root is exact (a perfect square: any correct sqrt returns it);
// an `if` on a literal condition keeps its live side.  `0 + x` stays an addition (x may be -0), `x * 0` with a
// per-pixel x stays a product.
// Rule: a loop is peeled when B0 has at most three quarters of the body's statements (assignments, phis and control
// statements, counted through nested blocks), i.e. at least a quarter of the first trip folds away; a loop whose first trip
// is no cheaper than any other only grows the kernel.
namespace {

struct Peel {
    using Map = std::map<const Value *, Primary>;
    FilterCode &code;
    std::map<const Value *, const Stmt *> if_of;      // exit phi of an `if` -> the if
    bool any = false;
    // counting pass of clone(): nothing is allocated, values the copy would define stay unmapped (an unmapped value is no
    // literal, like the copy's new value), so the same operations fold and `emitted` is what the real copy will have
    bool dry = false;

    explicit Peel(FilterCode &c) : code(c) { scan(c.body); }

    void scan(const Block &b) {
        for (const Stmt *s : b) {
            if (s->kind == Stmt::If) {
                for (const Stmt *ph : s->phis) if_of[ph->lhs] = s;
                scan(s->then_);
                scan(s->else_);
            } else if (s->kind == Stmt::While)
                scan(s->body);
        }
    }
    static bool is_lit(const Primary &p) { return p.kind == Primary::IntConst || p.kind == Primary::FloatConst; }
    static bool truthy(const Primary &p) { return p.kind == Primary::IntConst ? p.i != 0 : p.f != 0.0f; }

    // an operator on literals, exactly; the result converted like the assignment to a variable of type `lhs` does
    static bool fold_exact(const OpInfo *op, const std::vector<Primary> &a, Ty lhs, Primary &out) {
        if (!op->pure) return false;
        for (const Primary &p : a) if (!is_lit(p)) return false;
        if (!strcmp(op->cname, "sqrt") && a.size() == 1) {
            const double x = as_double(a[0]), r = std::sqrt(x);
            if (!(x >= 0.0) || r * r != x || (double)(float)r != r) return false;
            out = Primary::F((float)r);
        } else if (!fold_impl(op, a, out))
            return false;
        return convert_to(lhs, out);
    }
    // the value of `p` where it is a literal by exact folds of the straight-line code and the `if`s that define it
    bool const_eval(const Primary &p, Primary &out, int depth = 0) const {
        if (is_lit(p)) { out = p; return true; }
        if (p.kind != Primary::Val || depth > 64) return false;
        const Value *v = p.value;
        const Ty t = v->var->type;
        if (v->index < 0) { out = Primary::I(0); return convert_to(t, out); }      // uninitialised: reads as 0
        const Stmt *d = v->def;
        if (!d) return false;
        if (d->kind == Stmt::Assign && d->rhs.kind == Rhs::Prim) return const_eval(d->rhs.prim, out, depth + 1) && convert_to(t, out);
        if (d->kind == Stmt::Assign && d->rhs.kind == Rhs::Op) {
            std::vector<Primary> a(d->rhs.args.size());
            for (size_t i = 0; i < a.size(); ++i) if (!const_eval(d->rhs.args[i], a[i], depth + 1)) return false;
            return fold_exact(d->rhs.op, a, t, out);
        }
        auto it = if_of.find(v);
        if (d->kind != Stmt::Phi || it == if_of.end() || it->second->cond.kind != Rhs::Prim) return false;
        Primary c;
        if (!const_eval(it->second->cond.prim, c, depth + 1)) return false;
        const Rhs &side = truthy(c) ? d->rhs : d->rhs2;
        return side.kind == Rhs::Prim && const_eval(side.prim, out, depth + 1) && convert_to(t, out);
    }

    static int count(const Block &b) {
        int n = 0;
        for (const Stmt *s : b) {
            ++n;
            if (s->kind == Stmt::If) n += (int)s->phis.size() + count(s->then_) + count(s->else_);
            if (s->kind == Stmt::While) n += (int)s->phis.size() + count(s->body);
        }
        return n;
    }
    static Primary mapped(const Map &m, const Primary &p) {
        if (p.kind == Primary::Val) { auto it = m.find(p.value); if (it != m.end()) return it->second; }
        return p;
    }
    static Rhs mapped(const Map &m, const Rhs &r) {
        Rhs o = r;
        if (o.kind == Rhs::Prim) o.prim = mapped(m, o.prim);
        for (Primary &a : o.args) a = mapped(m, a);
        return o;
    }
    Stmt *new_def(Stmt::Kind k, const Stmt *like, Stmt *parent, Map &m) {
        Stmt *n = code.new_stmt(k);
        n->lhs = code.new_value(like->lhs->var);
        n->lhs->def = n;
        n->parent = parent;
        n->closure_id = like->closure_id;
        m[like->lhs] = Primary::V(n->lhs);
        return n;
    }
    // `lhs = p`: a literal that converts becomes the value itself, anything else a copy
    void bind(const Stmt *like, const Primary &p, Block &out, Stmt *parent, Map &m, int &emitted) {
        Primary lit = p;
        if (is_lit(p) && convert_to(like->lhs->var->type, lit)) { m[like->lhs] = lit; return; }
        ++emitted;
        if (dry) return;
        Stmt *n = new_def(Stmt::Assign, like, parent, m);
        n->rhs = Rhs::P(p);
        out.push_back(n);
    }
    // copies `b` with the operands mapped, folding what is exact; `emitted`: the statements the copy has
    void clone(const Block &b, Block &out, Stmt *parent, Map &m, int &emitted) {
        for (const Stmt *s : b) {
            if (s->kind == Stmt::Assign) {
                Rhs r = mapped(m, s->rhs);
                Primary lit;
                if (r.kind == Rhs::Prim) { bind(s, r.prim, out, parent, m, emitted); continue; }
                if (r.kind == Rhs::Op && fold_exact(r.op, r.args, s->lhs->var->type, lit)) { m[s->lhs] = lit; continue; }
                ++emitted;
                if (dry) continue;
                Stmt *n = new_def(Stmt::Assign, s, parent, m);
                n->rhs = r;
                out.push_back(n);
            } else if (s->kind == Stmt::If) {
                const Rhs c = mapped(m, s->cond);
                if (c.kind == Rhs::Prim && is_lit(c.prim)) {      // the live side, the exit phis as copies
                    const bool t = truthy(c.prim);
                    clone(t ? s->then_ : s->else_, out, parent, m, emitted);
                    for (const Stmt *ph : s->phis) bind(ph, mapped(m, t ? ph->rhs : ph->rhs2).prim, out, parent, m, emitted);
                    continue;
                }
                emitted += 1 + (int)s->phis.size();
                if (dry) {
                    clone(s->then_, out, parent, m, emitted);
                    clone(s->else_, out, parent, m, emitted);
                    continue;
                }
                Stmt *n = code.new_stmt(Stmt::If);
                n->parent = parent;
                n->cond = c;
                clone(s->then_, n->then_, n, m, emitted);
                clone(s->else_, n->else_, n, m, emitted);
                for (const Stmt *ph : s->phis) {
                    const Rhs a = mapped(m, ph->rhs), b2 = mapped(m, ph->rhs2);
                    Stmt *np = new_def(Stmt::Phi, ph, n, m);
                    np->rhs = a;
                    np->rhs2 = b2;
                    n->phis.push_back(np);
                }
                out.push_back(n);
            } else if (s->kind == Stmt::While) {
                emitted += 1 + (int)s->phis.size();
                if (dry) { clone(s->body, out, parent, m, emitted); continue; }
                Stmt *n = code.new_stmt(Stmt::While);
                n->parent = parent;
                std::vector<Stmt *> nps;
                for (const Stmt *ph : s->phis) {
                    const Rhs init = mapped(m, ph->rhs);      // evaluated in the enclosing scope
                    Stmt *np = new_def(Stmt::Phi, ph, n, m);
                    np->rhs = init;
                    n->phis.push_back(np);
                    nps.push_back(np);
                }
                n->cond = mapped(m, s->cond);
                clone(s->body, n->body, n, m, emitted);
                for (size_t i = 0; i < nps.size(); ++i) nps[i]->rhs2 = mapped(m, s->phis[i]->rhs2);
                out.push_back(n);
            }
        }
    }
    static bool plain(const Block &b) {      // only statements the copy knows how to make
        for (const Stmt *s : b) {
            if (s->kind == Stmt::Assign) { if (s->rhs.kind != Rhs::Prim && s->rhs.kind != Rhs::Op && s->rhs.kind != Rhs::Internal) return false; }
            else if (s->kind == Stmt::If) {
                if (!plain(s->then_) || !plain(s->else_)) return false;
                for (const Stmt *ph : s->phis) if (ph->rhs.kind != Rhs::Prim || ph->rhs2.kind != Rhs::Prim) return false;
            } else if (s->kind == Stmt::While) {
                if (!plain(s->body)) return false;
                for (const Stmt *ph : s->phis) if (ph->rhs.kind != Rhs::Prim || ph->rhs2.kind != Rhs::Prim) return false;
            } else
                return false;
        }
        return true;
    }
    bool peel(Stmt *w, Block &out) {
        if (w->cond.kind != Rhs::Prim || w->cond.prim.kind != Primary::Val || !plain(w->body)) return false;
        const Stmt *cph = nullptr;
        for (const Stmt *ph : w->phis) {
            if (ph->rhs.kind != Rhs::Prim || ph->rhs2.kind != Rhs::Prim) return false;
            if (ph->lhs == w->cond.prim.value) cph = ph;
        }
        Primary c0;
        if (!cph || !const_eval(cph->rhs.prim, c0) || !truthy(c0)) return false;      // not provably entered
        Map m0;
        for (const Stmt *ph : w->phis) {
            Primary init;
            m0[ph->lhs] = const_eval(ph->rhs.prim, init) ? init : ph->rhs.prim;
        }
        // the rule (above), on a counting pass: a loop that is not peeled leaves the code as it was, value numbers included
        Block b0;
        Map m = m0;
        int emitted = 0;
        dry = true;
        clone(w->body, b0, w->parent, m, emitted);
        dry = false;
        if (emitted * 4 > count(w->body) * 3) return false;
        m = m0;
        clone(w->body, b0, w->parent, m, emitted);
        for (Stmt *ph : w->phis) ph->rhs = Rhs::P(mapped(m, ph->rhs2.prim));
        for (Stmt *s : b0) out.push_back(s);
        return true;
    }
    void walk(Block &b) {
        Block out;
        for (Stmt *s : b) {
            if (s->kind == Stmt::If) { walk(s->then_); walk(s->else_); }
            if (s->kind == Stmt::While) {
                walk(s->body);
                if (peel(s, out)) any = true;
            }
            out.push_back(s);
        }
        b.swap(out);
    }
};

}  // namespace

bool peel_first_trips(FilterCode &code) {
    Peel p(code);
    p.walk(code.body);
    return p.any;
}

bool fold_constant_op(const OpInfo *op, const std::vector<Primary> &args, Primary &out) { return fold_impl(op, args, out); }

}  // namespace mm
