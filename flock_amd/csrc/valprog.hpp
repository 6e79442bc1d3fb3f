// Computed expressions of ProjectionExec / FilterExec in general (valprog.hip): what neither the column pass-through, q1's
// `literal * Int32 column` kernel nor the one-pass predicate program (pred.hpp) covers -- arithmetic over columns (+ - * / %, unary -),
// CAST / TRY_CAST between the numeric types, comparisons of computed values, CASE WHEN ... THEN ... ELSE ... END -- runs as ONE kernel
// per expression: the tree is flattened on the host into a postfix program (passed by value) and interpreted in the FLAG-TILE geometry
// of the selecting kernels (scan.hpp: 8192-row tiles, a lane's 32 rows = eight 16-byte loads per Int32 column).  Round 6: a pass of
// the program evaluates FOUR rows per lane (one 16-byte load per column operand, one scalar dispatch per operator and four rows), the top
// of the operand stack lives in registers (LDS only holds what waits below it), an operator whose right operand is a literal takes it as
// an immediate (no push, no pop), and division / remainder by a literal is a multiply-high by a host-made reciprocal (a 64-bit division is
// ~150 instructions per row on gfx950).  The filter form writes the flag words and wave counts the row-emitting machinery reads
// (no byte mask, no pass over one): profiles/r06/expr_*.
//
// Semantics restated from upstream DataFusion ~6 / arrow-rs ~8 (the fork's expressions/*.rs are not in the
// reference tree: ASSUMPTIONS, not pinned by reference-held vectors -- tests/test_plan_round5b.py checks them against the oracle's
// twin, oracle/generic_ops.py: eval_typed, and q1's reference-held projection stays on its own kernel):
//   A-V1 both operands of a binary operator have ONE type (the planner inserts the casts); an untyped literal takes the other side's;
//   A-V2 + - * and unary - on integers wrap at the type's width (arrow's unchecked kernels `add` / `subtract` / `multiply`); Float64 + - *
//        are IEEE (no contraction: -ffp-contract=off);
//   A-V3 / and %: arrow-rs `divide` / `modulus` = `math_checked_divide_op` (and `divide_scalar` / `modulus_scalar`, and the `simd` feature's
//        `simd_checked_divide` the fork enables, flock/Cargo.toml:12) test `is_zero()` on the divisor of every VALID row for EVERY native
//        type: a zero divisor -- integer 0, Float64 0.0 or -0.0 -- fails the whole call with ArrowError::DivideByZero.  (Arrow C++ /
//        pyarrow return +-inf / NaN for floats: a difference between the two Arrows, the fork runs arrow-rs.)  A NULL operand makes the
//        row NULL before the divisor is looked at.  Integer / and % truncate towards zero;
//   A-V4 INT_MIN / -1 and INT_MIN % -1 (Int32 and Int64): Rust's `/` and `%` panic ("attempt to divide with overflow"), and the fork's
//        release profile aborts on panic (Cargo.toml:27): the invocation dies.  Here: the call fails with FLOCKGPU_ERR_INVALID;
//   A-V5 CAST fails the call when a valid value does not fit the target (DataFusion casts with safe = false), TRY_CAST yields NULL;
//        Float64 -> integer truncates towards zero, NaN does not fit; integer -> Float64 rounds to nearest even;
//   A-V6 comparisons yield NULL when an operand is NULL; AND / OR / NOT are Kleene; IS [NOT] NULL never yields NULL;
//   A-V7 CASE evaluates every branch for every row (as the fork's CaseExpr does over the whole batch) and picks the first WHEN that is
//        TRUE, else ELSE, else NULL.
//
// Scalar functions (`scalar_function_expr`).  The fork's serde shape of ScalarFunctionExpr is not in the reference tree either; semantics are upstream
// DataFusion ~5/6's, i.e. Rust `f64` methods and chrono (ASSUMPTIONS, checked against tests/scalar_fn_ref.py and, there, against pyarrow.compute):
//   A-F1 the node is {"physical_expr": "scalar_function_expr", "name" | "fun": <name, any letter case>, "args": [<expr>, ...], "return_type": <data_type>};
//        a return_type that is not the function's result type is refused, a missing one is taken as the result type;
//   A-F2 a function of a NULL argument is NULL, and no function fails the call;
//   A-F3 math, Float64 -> Float64, one argument of static type Float64 (the planner casts): abs, signum, floor, ceil, round, trunc, sqrt are Rust's
//        f64::abs / signum / floor / ceil / round / trunc / sqrt: round takes halves away from zero; signum is 1.0 for +0.0 and +inf, -1.0 for -0.0
//        and -inf, NaN for NaN; abs(-0.0) = +0.0; floor / ceil / trunc keep the sign of a zero result; sqrt is the correctly rounded IEEE root
//        (NaN below zero, -0.0 for -0.0).  Every one of them is bit-exact on the device; exp, ln, log*, power and the trigonometric functions have no
//        bit-exact counterpart there and are refused;
//   A-F4 date_trunc(unit, ts) -> Timestamp(ms), unit a Utf8 literal among second, minute, hour, day, week (starts on Monday), month, year;
//        proleptic Gregorian calendar, UTC; before 1970 towards minus infinity (date_trunc('day', -1 ms) = -86 400 000);
//   A-F5 date_part(unit, ts) -> Int32, unit among year, month, day, hour, minute, second (whole seconds 0..59), dow (Sunday = 0), doy (from 1);
//   A-F6 ts is a Timestamp(ms) column or a Timestamp-valued function (date_trunc, now()); an Int64 value is not one;
//   A-F7 octet_length(s) -> Int32 bytes; char_length(s) = character_length = length -> Int32 code points = bytes that are not 10xxxxxx (strmatch.hpp
//        A-L2); s is a Utf8 column (a cast to Utf8 may sit in front).  A kernel per (column, function) writes the lengths as an Int32 column
//        (strlen.hip) which the program reads as any other column; the source's validity passes through;
//   A-F8 now() -> Timestamp(ms): the UTC wall clock, read once on the host when an execute begins; one value for every row and every occurrence.
//        The program holds it as a constant.
#pragma once
#include "relops.hpp"
#include "divmagic.hpp"

namespace flockgpu {

constexpr int kValMaxOps = 96;
constexpr int kValMaxCols = 8;
constexpr int kValMaxConsts = 32;
constexpr int kValMaxStack = 8;

enum class ValType : uint8_t { I32 = 0, I64 = 1, U64 = 2, F64 = 3, BOOL = 5, NONE = 255 };   // (0..3 = ColType)
enum class ValOpKind : uint8_t {
    Col = 0, Const, Null,                         // push
    Add, Sub, Mul, Div, Mod, Neg,                 // arithmetic in `type`
    Cast, TryCast,                                // `type` -> `to`
    Eq, Ne, Lt, Le, Gt, Ge,                       // compare in `type` -> BOOL
    And, Or, Not, IsNull, IsNotNull,              // BOOL (IsNull: any type)
    Select,                                       // pops THEN, WHEN, ELSE (pushed in the order ELSE, WHEN, THEN)
    Func                                          // a unary scalar function of the top: `to` = ValFn, `type` = the operand's type (F64 / I64)
};
// The device functions (A-F3..A-F5).  A program that holds one runs on the interpreter's kFunc instances (valprog.hip): the others keep their registers.
enum class ValFn : uint8_t {
    Abs = 0, Signum, Floor, Ceil, Round, Trunc, Sqrt,                                              // Float64 -> Float64
    TruncSecond, TruncMinute, TruncHour, TruncDay, TruncWeek, TruncMonth, TruncYear,             // Timestamp(ms) -> Timestamp(ms): + cal::Unit
    PartSecond, PartMinute, PartHour, PartDay, PartWeekUnused, PartMonth, PartYear, PartDow, PartDoy,   // Timestamp(ms) -> Int32: + cal::Unit
    kCount
};
struct ValOp {
    uint8_t kind, type, to, arg;   // ValOpKind; operand ValType; Cast target -- or, on a binary operator, kValImm: the right operand is consts[arg]
};                                 // (Div / Mod with kValImm: consts[arg] = divisor, [arg + 1] = reciprocal, [arg + 2] = shift | add << 8, [arg + 3]: see kValImm32; ValBuilder::fuse_immediate)
constexpr uint8_t kValImm = 0x80;
constexpr uint8_t kValImm32 = 0x81;   // Div / Mod by a literal |c| < 2^32 whose dividend is KNOWN to fit Int32 (ValBuilder::narrow): consts[arg + 3] = the 32-bit reciprocal
struct ValCol {
    const void *values;
    const uint8_t *valid;
    int32_t type;   // ColType
    int32_t pad;
};
struct ValProgram {
    ValCol cols[kValMaxCols];
    uint64_t consts[kValMaxConsts + 3];   // (+ 3: the interpreter fetches consts[arg .. arg + 3] for every operator ahead of its turn)
    ValOp ops[kValMaxOps];
    int32_t n_cols = 0, n_consts = 0, n_ops = 0, max_stack = 0;
};

// Host-side assembly (plan.hip walks the expression tree).  Every add returns false when the program is full.
struct ValBuilder {
    ValProgram p{};
    int depth = 0;
    uint32_t narrow = 0;   // bit i: the value in stack slot i is known to lie in [-2^31, 2^31) whatever its type (an Int32 column behind the planner's CAST to Int64, a small literal, a remainder of such)
    int add_col(const DevColumn &c) {
        for (int i = 0; i < p.n_cols; ++i)
            if (p.cols[i].values == c.values && p.cols[i].valid == c.valid) return i;
        if (p.n_cols >= kValMaxCols) return -1;
        p.cols[p.n_cols] = ValCol{c.values, c.valid, (int32_t)c.type, 0};
        return p.n_cols++;
    }
    int add_const(uint64_t bits) {
        for (int i = 0; i < p.n_consts; ++i)
            if (p.consts[i] == bits) return i;
        if (p.n_consts >= kValMaxConsts) return -1;
        p.consts[p.n_consts] = bits;
        return p.n_consts++;
    }
    // pops: operands the operator takes off the stack; every operator pushes one result
    bool push(ValOpKind k, ValType type, int pops, int arg = 0, ValType to = ValType::NONE) {
        if (p.n_ops >= kValMaxOps || arg < 0) return false;
        const bool fits = result_fits_i32(k, type, pops, arg, to);   // (looks at the operands: before anything moves)
        if (pops == 2 && fuse_immediate(k, type)) {
            set_narrow(depth - 1, fits);
            return true;
        }
        p.ops[p.n_ops++] = ValOp{(uint8_t)k, (uint8_t)type, (uint8_t)to, (uint8_t)arg};
        depth += 1 - pops;
        if (depth > p.max_stack) p.max_stack = depth;
        if (depth >= 1 && depth <= kValMaxStack) set_narrow(depth - 1, fits);
        return depth >= 1 && depth <= kValMaxStack;
    }
    // a unary function of the top of the stack (never fused with a literal: its operand is no Const the builder may take back)
    bool push_func(ValFn fn, ValType type) {
        if (p.n_ops >= kValMaxOps || depth < 1) return false;
        p.ops[p.n_ops++] = ValOp{(uint8_t)ValOpKind::Func, (uint8_t)type, (uint8_t)fn, 0};
        set_narrow(depth - 1, fn >= ValFn::PartSecond);   // (date_part: an Int32)
        return true;
    }
    void set_narrow(int slot, bool v) { narrow = v ? narrow | (1u << slot) : narrow & ~(1u << slot); }
    bool is_narrow(int slot) const { return slot >= 0 && ((narrow >> slot) & 1u); }
    // whether the operator's result is known to lie in the Int32 range (operands: slots depth - pops .. depth - 1)
    bool result_fits_i32(ValOpKind k, ValType type, int pops, int arg, ValType to) const {
        switch (k) {
            case ValOpKind::Col: return p.cols[arg].type == (int32_t)ColType::I32;
            case ValOpKind::Const: return type != ValType::F64 && (int64_t)p.consts[arg] >= INT32_MIN && (int64_t)p.consts[arg] <= INT32_MAX && !(type == ValType::U64 && (int64_t)p.consts[arg] < 0);
            case ValOpKind::Null: return true;
            case ValOpKind::Add: case ValOpKind::Sub: case ValOpKind::Mul: case ValOpKind::Neg: case ValOpKind::Div: return type == ValType::I32;   // (an Int32 result is wrapped to its width)
            case ValOpKind::Mod: return type == ValType::I32 || (type != ValType::F64 && is_narrow(depth - 2));   // |x % y| <= |x|
            case ValOpKind::Cast: case ValOpKind::TryCast: return to == ValType::I32 || (type != ValType::F64 && to != ValType::F64 && is_narrow(depth - 1) && !(to == ValType::U64));
            case ValOpKind::Select: return is_narrow(depth - 1) && is_narrow(depth - 3);   // THEN and ELSE
            default: return true;   // comparisons and logic: 0 / 1
        }
    }
    // A binary operator whose RIGHT operand was just pushed as a literal takes it as an immediate: the Const push goes, the operator
    // reads consts[arg].  Division / remainder by a non-zero integer literal get the reciprocal of |divisor| next to it (Granlund /
    // Montgomery, round-up variant, 64-bit: q = mulhi(n, m) >> s, or the 65-bit multiplier form ((n - hi) >> 1) + hi) >> s).
    bool fuse_immediate(ValOpKind k, ValType type) {
        if (p.n_ops < 1 || p.ops[p.n_ops - 1].kind != (uint8_t)ValOpKind::Const) return false;
        const bool arith = k == ValOpKind::Add || k == ValOpKind::Sub || k == ValOpKind::Mul || k == ValOpKind::Div || k == ValOpKind::Mod;
        const bool cmp = k == ValOpKind::Eq || k == ValOpKind::Ne || k == ValOpKind::Lt || k == ValOpKind::Le || k == ValOpKind::Gt || k == ValOpKind::Ge;
        if (!arith && !cmp) return false;
        int arg = p.ops[p.n_ops - 1].arg;
        uint8_t imm_kind = kValImm;
        const uint64_t c = p.consts[arg];
        if ((k == ValOpKind::Div || k == ValOpKind::Mod) && type != ValType::F64) {
            if (c == 0) return false;   // (a zero divisor: the generic operator reports it -- for the valid rows only)
            uint64_t d = c;
            if (type != ValType::U64 && (int64_t)c < 0) d = 0 - c;   // |divisor| (2^63 for INT64_MIN)
            uint64_t magic = 0, shift = 63, add = 0;
            while (!((d >> shift) & 1u)) --shift;   // floor(log2 d)
            if (d & (d - 1)) {
                const unsigned __int128 two = (unsigned __int128)1 << (64 + shift);
                unsigned __int128 pm = two / d;
                const unsigned __int128 rem = two - pm * d;
                if ((unsigned __int128)d - rem >= ((unsigned __int128)1 << shift)) {   // one more bit of multiplier
                    pm = pm * 2 + (rem * 2 >= d ? 1 : 0);
                    add = 1;
                }
                magic = (uint64_t)(pm + 1);
            }
            if (p.n_consts + 4 > kValMaxConsts) return false;
            arg = p.n_consts;
            p.consts[p.n_consts++] = c;
            p.consts[p.n_consts++] = magic;
            p.consts[p.n_consts++] = shift | (add << 8);
            // a dividend known to fit Int32 (the slot below the literal's) and |divisor| < 2^32: ONE 32 x 32 -> high-32 multiply per row
            // (divmagic.hpp) instead of the four of the 64-bit form
            uint64_t r32 = 0;
            if (d < (uint64_t(1) << 32) && is_narrow(depth - 2)) {
                const UMod32 m = umod32_make((uint32_t)d);
                r32 = (uint64_t)m.magic | ((uint64_t)m.shift << 32) | ((uint64_t)m.add << 40);
                imm_kind = kValImm32;
            }
            p.consts[p.n_consts++] = r32;
        }
        p.ops[p.n_ops - 1] = ValOp{(uint8_t)k, (uint8_t)type, imm_kind, (uint8_t)arg};
        depth -= 1;   // (the literal's push is taken back; the operator replaces its left operand in place)
        return true;
    }
};

// out_type: the value column's type (I32 / I64 / U64 / F64).  out_valid (may be null when the caller knows the result holds no NULL:
// then a NULL result is an error) receives one byte per row.  Error codes come back as FLOCKGPU_ERR_INVALID with the reason
// (division by zero / INT_MIN / -1 / a value that does not fit its CAST).  One host wait.
int valprog_to_column(flockgpu_ctx *ctx, const char *name, const ValProgram &prog, int64_t rows, ColType out_type, void *out_values, uint8_t *out_valid);
// FilterExec: the rows where the BOOL result is TRUE (FALSE and NULL: dropped), in order -- flag words + wave counts from the evaluating
// kernel itself, then the scan / emit of pred_to_rows.  One host wait (row count + error word).
int valprog_to_rows(flockgpu_ctx *ctx, const char *name, const ValProgram &prog, int64_t rows, int32_t **out_rows, int64_t *n_out);
// The predicate form's flag words and wave counts alone (pred.hpp pred_to_flags), for a consumer that reads the rows under them.  One host wait:
// the error word (a division by zero voids the call).
int valprog_to_flags(flockgpu_ctx *ctx, const char *name, const ValProgram &prog, int64_t rows, const uint32_t **flag_words, const uint32_t **wave_counts, int32_t *n_tiles);
// octet_length / char_length of a Utf8 column (A-F7; strlen.hip): one Int32 per row in an arena buffer called `name`, NULL rows included (their bytes are
// whatever the column holds: the consumer reads the source's validity).  No host wait.
// (range_begin / range_end, both or neither, code points only: the count inside [range_begin[i], range_end[i]) of the value -- an inner text slice)
int utf8_lengths(flockgpu_ctx *ctx, const char *name, const DevColumn &col, int64_t rows, bool code_points, int32_t **out, const int32_t *range_begin = nullptr,
                 const int32_t *range_end = nullptr);

}  // namespace flockgpu
