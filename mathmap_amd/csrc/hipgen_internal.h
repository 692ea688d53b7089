// Shared by the generator's two translation units: hipgen.cpp (the scalar generator and the translation unit's
// layout) and hipgen_pair.cpp (pair mode).  Not part of the interface (hipgen.h).
#pragma once
#include <functional>
#include <memory>
#include <optional>
#include <ostream>
#include <string>
#include <vector>

#include "hipgen.h"

namespace mm {
namespace hipgen {

enum Slice { PROLOGUE, PIXEL, ROWS };

// Every way the environment can alter the kernel text: hooks for experiments, never needed for correct operation.  One
// field per hook, read when the struct is made -- once per compile, by generate_hip; the generators of the filter
// functions get the same struct.  A valued hook is unset or an int (atoi of its text), a switch is set or not.
// (MMHIP_NO_CSE in passes.cpp and runtime.cpp's hooks do not change this text.)
std::optional<int> env_int(const char *name);      // the one place where the generator reads the environment
struct Knobs {
    std::optional<int> unroll = env_int("MMHIP_UNROLL");              // 1..8 pixels per loop step; set at all: no pair mode
    std::optional<int> tile_w = env_int("MMHIP_TILE_W");              // columns of a workgroup, instead of KernelOptions::tile_w
    std::optional<int> single_pixel = env_int("MMHIP_SINGLE_PIXEL");  // 1: one pixel per work-item, 0: the loop shape
    std::optional<int> pair = env_int("MMHIP_PAIR");                  // 0: never pair mode, 1: whenever the body is covered (unset: small bodies)
    bool pair_debug = env_int("MMHIP_PAIR_DEBUG").has_value();        // say on stderr why a body is not covered (same text)
    std::optional<int> pair_masks = env_int("MMHIP_PAIR_MASKS");      // #define MM_PAIR_MASKS; 0: truth values as ints, no exit-driven loops
    std::optional<int> pair_exit = env_int("MMHIP_PAIR_EXIT");        // 0: pair-mode loops keep the per-iteration selects
    // an exit-driven loop's back edge: 0 left to the compiler, 1 compare and mask (s_cmp, s_cselect_b64), unset / 2 counted (carry)
    std::optional<int> pair_exit_tail = env_int("MMHIP_PAIR_EXIT_TAIL");
    std::optional<int> pair_pack = env_int("MMHIP_PAIR_PACK");        // 0: pair kernels store through mm_store_pixel, a pixel at a time
    std::optional<int> pair_peel = env_int("MMHIP_PAIR_PEEL");        // 1: peel a first trip that folds off the loops of specialised pair kernels (pair_peel_enabled; default off: not measured yet)
    // 0: no fused doubling (hipgen_pair.cpp plan_fusion): `d = t + t; r = d + b` of an exit-driven loop stays two additions.
    // Only with the counted back edge: MMHIP_PAIR_EXIT=0 and MMHIP_PAIR_EXIT_TAIL=0 / 1 keep the earlier arithmetic whatever this says
    std::optional<int> pair_fma2 = env_int("MMHIP_PAIR_FMA2");
    // 0: the pair step as it was (hipgen_pair.cpp emit_pixel_loop): rows, clamp and 64-bit addresses per lane and step, a frame
    // constant's truth value through a vector compare.  Only with the fused doubling's conditions and without a peeled trip: every
    // earlier switch keeps its text whatever this says
    std::optional<int> pair_step = env_int("MMHIP_PAIR_STEP");
    // 0: a workgroup's steps are consecutive rows, as they were (hipgen_pair.cpp emit_pixel_loop): the single-frame kernel's text
    // as it was.  Only where the fast step is taken: MMHIP_PAIR_STEP=0 and every earlier switch keep their text whatever this says
    std::optional<int> pair_spread = env_int("MMHIP_PAIR_SPREAD");
    bool pair_no_uniform = env_int("MMHIP_PAIR_NO_UNIFORM").has_value();   // no wave-uniform scalars in pair-mode loops
    std::optional<int> nt_store = env_int("MMHIP_NT_STORE");          // #define MM_NT_STORE, instead of "the kernel fetches"
    std::optional<int> xcd_order = env_int("MMHIP_XCD_ORDER");        // workgroup -> tile order 0 / 1 / 2 (default 2)
    std::optional<int> waves_per_eu = env_int("MMHIP_WAVES_PER_EU");  // amdgpu_waves_per_eu attribute of the pixel kernel
    bool no_fetched_result = env_int("MMHIP_NO_FETCHED_RESULT").has_value();      // a pure distortion converts its fetch like any result
    bool no_same_taps = env_int("MMHIP_NO_SAME_TAPS").has_value();                // #define MM_NO_SAME_TAPS 1 (mm_device.h)
    bool no_outside_shortcut = env_int("MMHIP_NO_OUTSIDE_SHORTCUT").has_value();  // #define MM_NO_OUTSIDE_SHORTCUT 1 (mm_device.h)
    std::optional<int> frame_hot = env_int("MMHIP_FRAME_HOT");        // 0: a fetch with a per-pixel frame number is a generic fetch
    bool no_row_slice = env_int("MMHIP_NO_ROW_SLICE").has_value();    // no per-row kernel
    std::optional<int> max_call_depth = env_int("MMHIP_MAX_CALL_DEPTH");   // depth at which filter functions return zero (default 16)
};

// ---- pure helpers (hipgen.cpp) ----
std::string vname(const Value *v);              // the C variable of an SSA value
std::string ctype(const CompVar *v);
int type_size(const CompVar *v);
std::string float_literal(float f);
const char *libm_name(const char *cname, bool f32);
bool is_truth_op(const char *cname);            // LESS, LEQ, EQ, NOT: the operators whose value is 0 or 1
bool is_pow2_divisor(float c);                  // x / c is x * (1 / c), exactly: c = +-2^k, with room on both sides
bool nonneg_or_nan(const Value *v, int depth);  // is the float value provably >= +0 (or NaN)?
// `sqrt(a) < 2^k`, which is `0 <= a < 4^k` exactly: the operand a (a value) and 4^k; null for every other operation
const Primary *sqrt_less_pow2(const Rhs &r, float *kk);

// ---- pair mode (hipgen_pair.cpp) ----
// What pair mode sees of the scalar generator that hosts it.
struct PairEnv {
    std::ostream &out;
    FilterCode &code;
    const KernelOptions &opt;
    const Knobs &knobs;
    const std::vector<Value *> &pix_defs;                 // the values the pixel slice defines
    int pixel_stmts, pixel_fetches;                       // its size (pixel_stats)
    std::function<std::string(const Primary &)> prim;     // the scalar generator's text of an operand in the pixel slice ...
    std::function<std::string(const Stmt *)> rhs;         // ... and of an assignment's right-hand side
    std::function<bool(const Value *)> value_visible;     // can the pixel slice name the value?
    std::function<void(const std::string &, const std::string &)> emit_both;   // a text, and what stands in its place in the clip variant
};
struct PairMode {
    virtual ~PairMode() {}
    virtual bool exit_driven() const = 0;                 // loops in the exit-driven form (lane masks, MMHIP_PAIR_EXIT)
    virtual bool is_uniform(const Value *v) const = 0;    // kept as a wave-uniform scalar `u<name>` where the text now stands
    virtual void emit_helpers() = 0;                      // device functions of this kernel alone, behind the preludes
    virtual void emit_pixel_loop(const std::string &ind) = 0;   // the whole `for (; mm_p < A.ppt; mm_p += 2)` loop
};
// null: pair mode is not for this body (too large, fetches, a statement that is not covered, MMHIP_PAIR=0)
std::unique_ptr<PairMode> make_pair_mode(const PairEnv &env);

}  // namespace hipgen
}  // namespace mm
