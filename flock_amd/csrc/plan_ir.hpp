// Physical-plan IR of the plan-level C ABI (include/flockgpu_plan.h): the serde_json text of the reference's
// `Arc<dyn ExecutionPlan>` (flock/src/runtime/context.rs:477-480; dialect: SURVEY.md appendix C, fixtures
// flock/src/tests/data/plan/*.json) parsed into a small operator tree with derived schemas.  Host-side only.
//
// Kept nodes: memory_exec (Scan), filter_exec, projection_exec, hash_aggregate_exec, hash_join_exec,
// repartition_exec with Hash partitioning, sort_exec (ORDER BY over columns: the reference's own boundary goldens end in it,
// flock/src/runtime/context.rs:471,549; the splitter cuts stages at it, distributed_plan/stage.rs:337) and global_limit_exec /
// local_limit_exec.  coalesce_batches_exec, repartition_exec RoundRobinBatch, merge_exec / coalesce_partitions_exec change
// neither the row multiset nor the schema and are dropped.  window_agg_exec (Window) takes ROW_NUMBER() and
// COUNT / SUM / MIN / MAX / AVG over the default frame.  hash_join_exec takes join_type Inner, Semi and Anti (Semi / Anti: the left input's rows
// that have / lack a partner on the right, the left input's schema -- relops.hpp A-S1..6).  Anything else (other window functions and frames,
// Left / Right / Full joins, unknown expressions / types) makes the plan UNSUPPORTED: the host keeps its own engine for it.
// cross_join_exec (cross.hpp A-X1..6) is a Join node of JoinType::Cross without key pairs: left ++ right columns, L x R rows, pair (i, j) at row i * R + j.
// (The fork's typetag name cannot be checked -- its DataFusion source is not under the reference --: it follows the naming of every tag seen so far.)
// union_exec (union.hpp A-U1..7) is a Union node over `inputs`: UNION ALL, the inputs' rows one input after the other; a union directly under a union
// (also through the transparent nodes) is flattened, and in a plan that holds one the leaves of identical field lists share their `needed` masks.
// hash_aggregate_exec takes COUNT / SUM / MIN / MAX / AVG and COUNT(DISTINCT x) -- an aggr_expr entry tagged "distinct_count" (alias "count_distinct") with
// its one argument under `exprs` or `expr` (distinct.hpp A-D1..A-D7).  That aggregate's Partial state is a List column, which this boundary does not
// carry: Final / FinalPartitioned over the Partial of the same plan becomes ONE single-pass node over the Partial's input (Node::single_pass); a Partial
// with a distinct count that anything else consumes is refused.
// A computed expression ends in a number (the general evaluator, valprog.hpp) or in TEXT: a Utf8 literal, a Utf8 column or a CASE whose branches are such
// (textsel.hpp A-T1..A-T5) -- as a projected column and, through computed_column, as a GROUP BY / ORDER BY key or a COUNT / COUNT(DISTINCT) argument.
// The text slice functions split_part / left / right / ltrim / rtrim / btrim of a Utf8 column (textslice.hpp A-SL1..A-SL8) are text-valued expressions
// too: `split_part(url, '/', 4)`, `btrim(split_part(description, ',', 1))`.  Every other text-producing function stays refused.
// CAST(x AS Utf8) / TRY_CAST(x AS Utf8) of an Int32 / Int64 / UInt64 / Timestamp(ms) column or numeric expression (numtext.hpp A-NT1..A-NT7) is text-valued
// as well and counts as a Utf8 column wherever one is taken: `left(CAST(b_date_time AS Utf8), 10)` is NEXMark q10's date.
// CAST(s AS Int32 / Int64 / UInt64 / Timestamp(ms)) / TRY_CAST of a text-valued expression (textnum.hpp A-TN1..A-TN6) is the way back: a numeric value of
// the general evaluator, `CAST(left(credit_card, 4) AS Int32)`.  Float64, Boolean, another Timestamp unit and a literal operand are refused by name.
#pragma once
#include <algorithm>
#include <cctype>
#include <set>
#include <sstream>

#include "plan_json.hpp"
#include "relops.hpp"
#include "strmatch.hpp"
#include "textsel.hpp"
#include "textslice.hpp"

namespace flockgpu {
namespace ir {

struct Field {
    std::string name;
    ColType type = ColType::I32;
    bool is_ts = false;
    bool nullable = false;
};

// Expression dialect (SURVEY.md appendix C + the unary / list expressions of the fork's expressions/*.rs, upstream DataFusion ~6:
// IsNullExpr{arg}, IsNotNullExpr{arg}, NotExpr{arg}, NegativeExpr{arg}, InListExpr{expr, list, negated}).
enum class EKind { Col, LitI, LitF, LitS, LitB, LitNull, Bin, Cast, Not, IsNull, IsNotNull, Neg, InList, Case, Func };
// Scalar functions (`scalar_function_expr`; shape and semantics: valprog.hpp A-F1..A-F8)
// ... and the text slice functions (textslice.hpp A-SL1..A-SL8), SplitPart .. Btrim in SliceFn's order
enum class Fn { Abs, Signum, Floor, Ceil, Round, Trunc, Sqrt, DateTrunc, DatePart, OctetLength, CharLength, Now, SplitPart, Left, Right, Ltrim, Rtrim, Btrim };
struct Expr {
    EKind kind = EKind::Col;
    int col = -1;  // Col: index into the input schema
    int64_t i = 0;   // LitI value / LitB 0 | 1
    double f = 0;
    std::string s;   // LitS value / Bin operator (Rust enum ident: Eq, NotEq, Lt, LtEq, Gt, GtEq, And, Or, Modulo, Multiply, Like, NotLike)
    ColType cast_to = ColType::I64;
    std::unique_ptr<Expr> l, r;  // Bin operands; the operand of Cast / Not / IsNull / IsNotNull / Neg / InList in l
    std::vector<std::unique_ptr<Expr>> list;   // InList: the literals; Case: WHEN, THEN, WHEN, THEN, ... (base expression in l, ELSE in r; either may be null)
    bool negated = false;                      // InList: NOT IN
    bool big_unsigned = false;                 // LitI: `i` is the bit pattern of a UInt64 above INT64_MAX
    bool cast_ts = false;                      // Cast: the target is Timestamp(Millisecond) (Int64 storage)
    bool try_cast = false;                     // Cast: try_cast_expr (a value that does not fit becomes NULL instead of failing the call)
    bool num_text = false;                     // Cast to Utf8 of something that is not text: the number / timestamp is FORMATTED (numtext.hpp); false: Utf8 to Utf8, nothing happens
    bool text_num = false;                     // Cast of a text-valued expression to Int32 / Int64 / UInt64 / Timestamp(ms): the text is PARSED (textnum.hpp)
    std::string lit_kind;                      // literals: the ScalarValue variant ("Int32", "Float64", ...; empty: a bare JSON value)
    Fn fn = Fn::Abs;                           // Func: the function (`s`: its canonical name; `i`: the cal::Unit of date_trunc / date_part, else -1; `list`: the value
                                               // arguments -- one, none for now(); the unit literal is folded into `i`)
    int64_t slice_n = 0;                       // Func, a slice function: split_part's field, left's / right's count
    std::string slice_arg;                     // Func, a slice function: split_part's delimiter, the trims' characters (`slice_has_arg`: written in the call)
    bool slice_has_arg = false;
};
inline bool fn_is_math(Fn f) { return f <= Fn::Sqrt; }
inline bool fn_is_slice(Fn f) { return f >= Fn::SplitPart; }
inline SliceFn slice_fn_of(Fn f) { return (SliceFn)((int)f - (int)Fn::SplitPart); }
// A slice call as text, the way explain prints it: split_part(url, '/', 4), btrim(split_part(description, ',', 1)), ltrim(name).  Identical calls
// give identical text: the key under which one source table holds a slice once.  (`e` a slice Func; a cast in front of the value argument is not printed.)
// (A value argument that is a cast of a number to Utf8 -- numtext.hpp -- prints as CAST(price AS Utf8): expr_text below.)
inline std::string expr_text(const Expr *e, const std::vector<std::string> &col_names);
inline std::string slice_text(const Expr *e, const std::vector<std::string> &col_names) {
    const Expr *v = e->list[0].get();
    while (v->kind == EKind::Cast && !v->num_text) v = v->l.get();
    std::string t = e->s + "(";
    if (v->kind == EKind::Cast) t += expr_text(v, col_names);
    else if (v->kind == EKind::Func) t += slice_text(v, col_names);
    else if (v->kind == EKind::Col && v->col >= 0 && (size_t)v->col < col_names.size()) t += col_names[(size_t)v->col];
    else t += "#" + std::to_string(v->col);
    if (e->slice_has_arg) t += ", '" + e->slice_arg + "'";
    if (e->fn == Fn::SplitPart || e->fn == Fn::Left || e->fn == Fn::Right) t += ", " + std::to_string(e->slice_n);
    return t + ")";
}
// An expression as text, structure for structure: identical expressions give identical text -- the key under which a source table holds the cast of a
// number to Utf8 once -- and explain prints it (CAST(price * 2 AS Utf8)).
inline std::string expr_text(const Expr *e, const std::vector<std::string> &col_names) {
    if (!e) return "?";
    auto list = [&](const char *sep) {
        std::string t;
        for (size_t i = 0; i < e->list.size(); ++i) t += (i ? sep : "") + expr_text(e->list[i].get(), col_names);
        return t;
    };
    static const char *types[] = {"Int32", "Int64", "UInt64", "Float64", "Utf8"};
    switch (e->kind) {
        case EKind::Col: return e->col >= 0 && (size_t)e->col < col_names.size() ? col_names[(size_t)e->col] : "#" + std::to_string(e->col);
        case EKind::LitI: return e->big_unsigned ? std::to_string((uint64_t)e->i) : std::to_string(e->i);
        case EKind::LitF: { std::ostringstream os; os << e->f; return os.str(); }
        case EKind::LitS: return "'" + e->s + "'";
        case EKind::LitB: return e->i ? "TRUE" : "FALSE";
        case EKind::LitNull: return "NULL";
        case EKind::Cast:
            return std::string(e->try_cast ? "TRY_CAST(" : "CAST(") + expr_text(e->l.get(), col_names) + " AS " + (e->cast_ts ? "Timestamp(ms)" : types[(int)e->cast_to <= 4 ? (int)e->cast_to : 4]) + ")";
        case EKind::Neg: return "-(" + expr_text(e->l.get(), col_names) + ")";
        case EKind::Not: return "NOT (" + expr_text(e->l.get(), col_names) + ")";
        case EKind::IsNull: return "(" + expr_text(e->l.get(), col_names) + ") IS NULL";
        case EKind::IsNotNull: return "(" + expr_text(e->l.get(), col_names) + ") IS NOT NULL";
        case EKind::InList: return "(" + expr_text(e->l.get(), col_names) + (e->negated ? ") NOT IN (" : ") IN (") + list(", ") + ")";
        case EKind::Bin: return "(" + expr_text(e->l.get(), col_names) + " " + e->s + " " + expr_text(e->r.get(), col_names) + ")";
        case EKind::Func:
            if (fn_is_slice(e->fn)) return slice_text(e, col_names);
            return e->s + "(" + (e->i >= 0 ? std::to_string(e->i) + ", " : std::string()) + list(", ") + ")";
        case EKind::Case:
            return "CASE " + (e->l ? expr_text(e->l.get(), col_names) + " " : std::string()) + "[" + list("; ") + "]" + (e->r ? " ELSE " + expr_text(e->r.get(), col_names) : std::string()) + " END";
    }
    return "?";
}
// how deep slice calls nest in `e` (a column, or a number cast to Utf8: 0)
inline int slice_depth(const Expr *e) {
    while (e->kind == EKind::Cast && !e->num_text) e = e->l.get();
    return e->kind == EKind::Func && fn_is_slice(e->fn) ? 1 + slice_depth(e->list[0].get()) : 0;
}
// the result is a Timestamp(Millisecond): CAST(x AS Timestamp), date_trunc, now()
inline bool expr_is_ts(const Expr *e) {
    return (e->kind == EKind::Cast && e->cast_ts) || (e->kind == EKind::Func && (e->fn == Fn::DateTrunc || e->fn == Fn::Now));
}

// Static type of an expression over `schema`: 0..3 = ColType I32 / I64 / U64 / F64, 4 = Utf8, 5 = Boolean, -1 = an untyped literal (it takes
// the type of whatever it meets), -2 = no consistent type.  (valprog.hpp: both operands of a binary operator have one type.)
inline int expr_static_type(const Expr *e, const std::vector<Field> &schema) {
    auto arith = [](const std::string &op) { return op == "Plus" || op == "Minus" || op == "Multiply" || op == "Divide" || op == "Modulo"; };
    switch (e->kind) {
        case EKind::Col: return e->col >= 0 && (size_t)e->col < schema.size() ? (int)schema[(size_t)e->col].type : -2;
        case EKind::LitI: return e->lit_kind == "Int32" ? 0 : e->lit_kind == "Int64" ? 1 : e->lit_kind == "UInt64" ? 2 : -1;
        case EKind::LitF: return 3;
        case EKind::LitS: return 4;
        case EKind::LitB: return 5;
        case EKind::LitNull: return e->lit_kind == "Utf8" ? 4 : -1;   // ({"Utf8": null} is a NULL of type Utf8, textsel.hpp A-T1; every other NULL takes the type it meets)
        case EKind::Cast: return (int)e->cast_to;
        case EKind::Neg: return expr_static_type(e->l.get(), schema);
        case EKind::Not: case EKind::IsNull: case EKind::IsNotNull: case EKind::InList: return 5;
        case EKind::Bin: {
            if (!arith(e->s)) return 5;
            const int a = expr_static_type(e->l.get(), schema), b = expr_static_type(e->r.get(), schema);
            if (a == -2 || b == -2 || a >= 4 || b >= 4) return -2;
            if (a == -1) return b;
            if (b == -1 || a == b) return a;
            // (fixtures of older fork revisions write q1's conversion as `Float64 literal * Int32 column` without the cast the planner inserts)
            if (e->s == "Multiply" && (e->l->kind == EKind::LitF || e->r->kind == EKind::LitF)) return 3;
            return -2;
        }
        case EKind::Func: return fn_is_slice(e->fn) ? 4 : fn_is_math(e->fn) ? 3 : (e->fn == Fn::DateTrunc || e->fn == Fn::Now) ? 1 : 0;
        case EKind::Case: {
            int t = -1;
            for (size_t i = 1; i < e->list.size() && t == -1; i += 2) t = expr_static_type(e->list[i].get(), schema);
            if (t == -1 && e->r) t = expr_static_type(e->r.get(), schema);
            return t;
        }
    }
    return -2;
}

enum class NKind { Scan, Filter, Project, Aggregate, Join, Repartition, Sort, Limit, Window, Union };
struct SortCol {
    int col = -1;            // input column
    bool descending = false;
    bool nulls_first = false;  // parsed and carried; device columns hold no NULLs (a NULL that could reach a sort is refused at feed)
};
// Aggregate functions and stage modes: a name becomes its enum once, where the parser validates it (parse_agg_fn / parse_agg_mode)
enum class AggFn { Count, Sum, Min, Max, Avg, CountDistinct };
enum class AggMode { Partial, Final, FinalPartitioned };
inline const char *agg_fn_name(AggFn f) {   // the lower-case name, as the messages print it
    static const char *names[] = {"count", "sum", "min", "max", "avg", "distinct_count"};
    return names[(int)f];
}
inline const char *agg_mode_name(AggMode m) {
    static const char *names[] = {"Partial", "Final", "FinalPartitioned"};
    return names[(int)m];
}
// (the five ordinary functions, GROUP BY's and the window aggregates'; a distinct count is recognised by is_distinct_count_tag, in hash_aggregate_exec alone)
inline bool parse_agg_fn(const std::string &name, AggFn *out) {
    for (AggFn f : {AggFn::Count, AggFn::Sum, AggFn::Min, AggFn::Max, AggFn::Avg})
        if (name == agg_fn_name(f)) { *out = f; return true; }
    return false;
}
inline bool parse_agg_mode(const std::string &name, AggMode *out) {
    for (AggMode m : {AggMode::Partial, AggMode::Final, AggMode::FinalPartitioned})
        if (name == agg_mode_name(m)) { *out = m; return true; }
    return false;
}
inline bool is_distinct_count_tag(const std::string &name) { return name == "distinct_count" || name == "count_distinct"; }
inline bool agg_is_minmax(AggFn f) { return f == AggFn::Min || f == AggFn::Max; }
// The argument types an aggregate takes -- in GROUP BY, without one and as a window function: COUNT any column, MIN / MAX integers and Float64,
// SUM / AVG integers, a distinct count integers and Utf8.  Every check of an argument's type, at create and at execute, asks here.
inline bool agg_takes(AggFn f, ColType t) {
    if (t == ColType::UTF8) return f == AggFn::Count || f == AggFn::CountDistinct;
    if (t == ColType::F64) return f == AggFn::Count || agg_is_minmax(f);
    return true;
}
// The 64-bit accumulator of COUNT / SUM / MIN / MAX over a column of type `t` (GROUP BY's and the window aggregates'; AVG: its sum -- the count
// beside it is the caller's)
inline AggOp agg_op_for(AggFn f, ColType t) {
    const bool uns = t == ColType::U64, f64 = t == ColType::F64;
    switch (f) {
        case AggFn::Count: return AggOp::COUNT;
        case AggFn::Max: return f64 ? AggOp::MAX_F64 : uns ? AggOp::MAX_U : AggOp::MAX_S;
        case AggFn::Min: return f64 ? AggOp::MIN_F64 : uns ? AggOp::MIN_U : AggOp::MIN_S;
        default: return AggOp::SUM_INT;
    }
}
struct Agg {
    AggFn fn = AggFn::Count;
    int arg = -1;    // Partial: input column of the argument (-1: a literal, COUNT(UInt8(1))); Final: the first state column
    int arg2 = -1;   // Final AVG: its second state column (the sum; `arg` is the count)
    std::string name;
    ColType type = ColType::U64;  // type of the finished aggregate
};
// State columns a Partial stage emits per aggregate, as DataFusion ~6 lays them out (Accumulator::state / state_fields,
// SURVEY.md appendix D): COUNT -> [count UInt64]; MAX / MIN / SUM -> [value]; AVG -> [count UInt64, sum Float64].
// (COUNT(DISTINCT) never emits its state: one result column in the single-pass node, Node::single_pass)
inline int agg_state_cols(AggFn fn) { return fn == AggFn::Avg ? 2 : 1; }
// 64-bit accumulators the aggregate takes in GROUP BY's table / the ungrouped reduce: a distinct count takes none, it owns a table of its own
inline int agg_accumulators(AggFn fn) { return fn == AggFn::CountDistinct ? 0 : agg_state_cols(fn); }
constexpr int kMaxDistinctCounts = 4;          // of one aggregate node
constexpr int kMaxUngroupedAccumulators = 8;   // of one aggregate without GROUP BY (AVG takes two)
constexpr int kMaxGroupedAccumulators = 16;    // of one GROUP BY (AVG takes two): groupwide.hpp kMaxWideAggs
// key pairs of one HashJoinExec (the composite-key path, relops.hpp key_codes, takes up to eight columns)
constexpr int kMaxJoinPairs = 8;
// One column of a WindowAggExec: ROW_NUMBER(), or an aggregate over the default frame (RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW: the
// partition's rows up to the last PEER of the current row -- equal ORDER BY values; the whole partition without ORDER BY).
struct WinExpr {
    bool row_number = true;
    AggFn fn = AggFn::Count;       // aggregate: the function
    int arg = -1;                  // aggregate: input column of the argument (-1: COUNT(*))
    ColType type = ColType::U64;   // the window column's type (the aggregate's data_type; COUNT UInt64, AVG Float64)
    bool is_ts = false;            // MIN / MAX of a Timestamp
    std::vector<int> part;         // input columns of the PARTITION BY
    std::vector<SortCol> order;    // aggregate: input columns of the ORDER BY (they delimit the peer groups; the input arrives sorted)
};
constexpr int kMaxUnionInputs = 64;   // inputs of one union_exec after flattening (union.hpp kUnionMaxInputs)
constexpr int kMaxWindowKeys = 4;   // PARTITION BY / ORDER BY columns of an aggregate window (each)
enum class JoinType { Inner, Semi, Anti, Cross };   // Cross: cross_join_exec -- no key pairs (`on` empty), every pair of rows
// a join key pair that can compare: two Utf8 columns, or two integer columns of one signedness (Float64 keys are refused)
inline bool join_keys_comparable(ColType x, ColType y) {
    return x != ColType::F64 && y != ColType::F64 && (x == ColType::UTF8) == (y == ColType::UTF8) && (x == ColType::U64) == (y == ColType::U64);
}
struct KeyPair { int l = -1, r = -1; };   // one `left column = right column` of a join
struct Node {
    NKind kind = NKind::Scan;
    int id = 0;
    std::vector<std::unique_ptr<Node>> in;
    std::vector<Field> schema;
    int leaf = -1;                  // Scan: index into Plan::leaves
    std::unique_ptr<Expr> pred;     // Filter
    std::vector<std::pair<std::unique_ptr<Expr>, std::string>> proj;  // Project
    AggMode mode = AggMode::Partial;   // Aggregate
    std::vector<int> group;         // Aggregate: input columns of the group keys
    std::vector<Agg> aggs;
    // Aggregate with a distinct count: Final / FinalPartitioned and the Partial below it as ONE aggregation over the Partial's input -- `mode` is the
    // upper node's, arguments are input columns as a Partial's, the schema is the finished results' (AVG one Float64 column)
    bool single_pass = false;
    std::vector<KeyPair> on;        // Join: the key pairs, 1 to kMaxJoinPairs (q9 has two: auction = id AND price = final); none for JoinType::Cross
    bool join_partitioned = false;  // Join: mode=Partitioned (both inputs arrive hash-partitioned on the keys)
    JoinType join_type = JoinType::Inner;   // Join: Semi / Anti return rows of the LEFT input only (schema = the left input's)
    std::vector<int> hash_cols;     // Repartition
    int n_parts = 0;
    bool hash_diff = false;         // Repartition: HashDiff -- one partition per DISTINCT key (n_parts = what the host counted)
    std::vector<SortCol> sort_cols; // Sort: ORDER BY keys, most significant first
    int64_t limit = -1;             // Limit: rows kept
    std::vector<WinExpr> win;       // Window: one per window column (they come FIRST in the schema)
    std::vector<char> required;     // per output column: needed by an ancestor (or by the plan output)
};

// Aggregate without GROUP BY: a lone MAX over one integer column (q5 / q7's MAX(num)) keeps the path and the feed-time NULL dropping it has had
// from the start; every other list of aggregates is one streaming pass (reduce.hpp).
inline bool lone_integer_max(const Node *n) {
    if (!n->group.empty() || n->aggs.size() != 1 || n->aggs[0].fn != AggFn::Max || n->aggs[0].arg < 0 || n->in.empty()) return false;
    const std::vector<Field> &sch = n->in[0]->schema;
    if ((size_t)n->aggs[0].arg >= sch.size()) return false;
    const ColType at = sch[(size_t)n->aggs[0].arg].type;
    return at != ColType::UTF8 && at != ColType::F64;
}
inline bool has_distinct_count(const Node *n) {
    for (auto &a : n->aggs)
        if (a.fn == AggFn::CountDistinct) return true;
    return false;
}
inline int node_accumulators(const Node *n) {
    int accs = 0;
    for (auto &a : n->aggs) accs += agg_accumulators(a.fn);
    return accs;
}

struct Leaf {
    std::vector<Field> schema;  // the columns the MemoryExec scans (after its projection)
    std::string relation;       // bid | auction | person | side_input | "" (guessed from the column names)
    std::vector<char> needed;   // per column: read by the plan (others are never uploaded)
    // per column: a row whose value here is NULL can be dropped at the scan without changing the plan's result (the column
    // only feeds inner-join keys, MAX arguments or comparisons) -- how the NULL `maxn` of an empty partition is ingested
    std::vector<char> null_droppable;
    // the leaf feeds a HashJoinExec mode=Partitioned / a FinalPartitioned aggregate without a hash repartition of this plan in
    // between: its batches were placed by the PRODUCING stage's hash, and every such leaf of the plan must have been placed by
    // the same one (flockgpu_plan.h "hash placement")
    bool co_partitioned = false;
};

struct Plan {
    std::unique_ptr<Node> root;
    std::vector<Leaf> leaves;
    int n_nodes = 0;
    std::string why;  // reason when unsupported
    bool has_union = false;   // a union_exec somewhere: leaves of identical field lists share their `needed` masks (union.hpp A-U7)
};

// ---------------------------------------------------------------------------------------------------------------------
inline const std::string &tag(const JValue *n) {
    static const std::string empty;
    const JValue *t = n ? n->get("execution_plan") : nullptr;
    return t && t->kind == JValue::Str ? t->str : empty;
}
inline const std::string &etag(const JValue *e) {
    static const std::string empty;
    const JValue *t = e ? e->get("physical_expr") : nullptr;
    return t && t->kind == JValue::Str ? t->str : empty;
}

inline bool parse_type(const JValue *dt, ColType *t, bool *is_ts) {
    *is_ts = false;
    if (!dt) return false;
    if (dt->kind == JValue::Str) {
        if (dt->str == "Int32") { *t = ColType::I32; return true; }
        if (dt->str == "Int64") { *t = ColType::I64; return true; }
        if (dt->str == "UInt64") { *t = ColType::U64; return true; }
        if (dt->str == "Float64") { *t = ColType::F64; return true; }
        if (dt->str == "Utf8") { *t = ColType::UTF8; return true; }
        return false;
    }
    if (dt->kind == JValue::Obj && dt->obj.size() == 1 && dt->obj[0].first == "Timestamp") {
        const JValue *a = dt->obj[0].second.get();
        if (a->kind == JValue::Arr && !a->arr.empty() && a->arr[0]->kind == JValue::Str && a->arr[0]->str == "Millisecond") {
            *t = ColType::I64;
            *is_ts = true;
            return true;
        }
    }
    return false;
}

inline const char *type_name(const Field &f) {
    if (f.is_ts) return "Timestamp(ms)";
    switch (f.type) {
        case ColType::I32: return "Int32";
        case ColType::I64: return "Int64";
        case ColType::U64: return "UInt64";
        case ColType::F64: return "Float64";
        default: return "Utf8";
    }
}

struct Builder {
    Plan *plan;
    std::string err;
    bool fail(const std::string &m) {
        if (err.empty()) err = m;
        return false;
    }

    // hash_aggregate_exec `j` lists a distinct count
    static bool json_has_distinct_count(const JValue *j) {
        const JValue *ae = j->get("aggr_expr");
        if (ae && ae->kind == JValue::Arr)
            for (auto &x : ae->arr)
                if (x->kind == JValue::Obj && is_distinct_count_tag(x->s("aggregate_expr"))) return true;
        return false;
    }
    // The Partial hash_aggregate_exec that Final / FinalPartitioned `j` merges: below nothing but repartition_exec / coalesce_* / merge_exec nodes, with
    // as many group keys and the same aggregates by tag and name.  Null: there is none.
    static const JValue *partial_below(const JValue *j) {
        const JValue *c = j->get("input");
        for (int depth = 0; c && c->kind == JValue::Obj && depth < 64; ++depth) {
            const std::string &t = tag(c);
            if (t != "repartition_exec" && t != "coalesce_batches_exec" && t != "coalesce_partitions_exec" && t != "merge_exec") break;
            c = c->get("input");
        }
        if (!c || c->kind != JValue::Obj || tag(c) != "hash_aggregate_exec" || c->s("mode") != "Partial") return nullptr;
        auto count = [](const JValue *l) { return l && l->kind == JValue::Arr ? l->arr.size() : (size_t)0; };
        const JValue *ga = j->get("group_expr"), *gb = c->get("group_expr"), *aa = j->get("aggr_expr"), *ab = c->get("aggr_expr");
        if (count(ga) != count(gb) || count(aa) != count(ab)) return nullptr;
        for (size_t i = 0; i < count(aa); ++i) {
            const JValue *x = aa->arr[i].get(), *y = ab->arr[i].get();
            if (x->kind != JValue::Obj || y->kind != JValue::Obj || x->s("name") != y->s("name")) return nullptr;
            const std::string fx = x->s("aggregate_expr"), fy = y->s("aggregate_expr");
            if (fx != fy && !(is_distinct_count_tag(fx) && is_distinct_count_tag(fy))) return nullptr;
        }
        return c;
    }

    bool fields_of(const JValue *schema, std::vector<Field> *out) {
        const JValue *fields = schema ? schema->get("fields") : nullptr;
        if (!fields || fields->kind != JValue::Arr) return fail("node without schema.fields");
        for (auto &f : fields->arr) {
            Field fd;
            fd.name = f->s("name");
            const JValue *nl = f->get("nullable");
            fd.nullable = nl && nl->kind == JValue::Bool && nl->b;
            if (!parse_type(f->get("data_type"), &fd.type, &fd.is_ts)) return fail("column '" + fd.name + "': data type outside {Int32, Int64, UInt64, Float64, Utf8, Timestamp(ms)}");
            out->push_back(fd);
        }
        return true;
    }

    // column{name[,index]} against `schema`: by index when it names the same column, else by name (older fork
    // revisions serialise the name only)
    int resolve(const JValue *e, const std::vector<Field> &schema) {
        const std::string name = e->s("name");
        const JValue *ix = e->get("index");
        if (ix && ix->kind == JValue::Num && ix->is_int && ix->inum >= 0 && (size_t)ix->inum < schema.size() &&
            (name.empty() || schema[(size_t)ix->inum].name == name))
            return (int)ix->inum;
        for (size_t i = 0; i < schema.size(); ++i)
            if (schema[i].name == name) return (int)i;
        // qualified name ("bid.price", "CountBids.num") against an unqualified schema
        const size_t dot = name.rfind('.');
        if (dot != std::string::npos)
            for (size_t i = 0; i < schema.size(); ++i)
                if (schema[i].name == name.substr(dot + 1)) return (int)i;
        return -1;
    }

    std::unique_ptr<Expr> expr(const JValue *e, const std::vector<Field> &schema) {
        std::unique_ptr<Expr> x(new Expr());
        const std::string &t = etag(e);
        if (t == "column") {
            x->kind = EKind::Col;
            x->col = resolve(e, schema);
            if (x->col < 0) { fail("column '" + e->s("name") + "' not in the input schema"); return nullptr; }
            return x;
        }
        if (t == "literal") {
            const JValue *val = e->get("value");
            std::string kind;
            if (val && val->kind == JValue::Obj && val->obj.size() == 1) {
                kind = val->obj[0].first;
                val = val->obj[0].second.get();
            }
            if (!val) { fail("literal without value"); return nullptr; }
            x->lit_kind = kind;
            if (val->kind == JValue::Null) { x->kind = EKind::LitNull; return x; }   // ScalarValue::Int32(None) and its siblings
            if (val->kind == JValue::Bool) { x->kind = EKind::LitB; x->i = val->b ? 1 : 0; return x; }
            if (val->kind == JValue::Str) { x->kind = EKind::LitS; x->s = val->str; return x; }
            if (val->kind == JValue::Num) {
                if (val->is_int && kind.find("Float") == std::string::npos) { x->kind = EKind::LitI; x->i = val->inum; x->big_unsigned = val->is_big_unsigned; }
                else { x->kind = EKind::LitF; x->f = val->num; }
                return x;
            }
            fail("literal of an unsupported kind");
            return nullptr;
        }
        if (t == "cast_expr" || t == "try_cast_expr") {
            x->kind = EKind::Cast;
            x->try_cast = t == "try_cast_expr";
            bool ts = false;
            if (!parse_type(e->get("cast_type"), &x->cast_to, &ts)) {
                // of text, by name (textnum.hpp A-TN5); everything else as before
                const std::string before = err;
                const JValue *ct = e->get("cast_type");
                auto op = expr(e->get("expr"), schema);
                const bool text = op && err == before && expr_static_type(op.get(), schema) == 4;
                err = before;
                if (text && ct && ct->kind == JValue::Str && ct->str == "Boolean") fail(t + ": CAST of a Utf8 value to Boolean (no Boolean columns at this boundary)");
                else if (text && ct && ct->kind == JValue::Obj && ct->obj.size() == 1 && ct->obj[0].first == "Timestamp")
                    fail(t + ": CAST of a Utf8 value to a Timestamp of another unit than Millisecond (the text is parsed to Timestamp(Millisecond, None) alone)");
                else fail("cast to an unsupported type");
                return nullptr;
            }
            x->cast_ts = ts;
            x->l = expr(e->get("expr"), schema);
            if (!x->l) return nullptr;
            if ((int)x->cast_to <= 3 && expr_static_type(x->l.get(), schema) == 4) {   // text to a number or a timestamp: the value is parsed (textnum.hpp)
                const Expr *v = x->l.get();
                while (v->kind == EKind::Cast && v->cast_to == ColType::UTF8 && !v->num_text) v = v->l.get();
                if (v->kind == EKind::LitS || v->kind == EKind::LitNull) { fail(t + ": CAST of a Utf8 literal to a number (a literal operand: write the number itself)"); return nullptr; }
                if (x->cast_to == ColType::F64) {
                    fail(t + ": CAST of a Utf8 value to Float64 (no correctly rounded decimal-to-double conversion on the device)");
                    return nullptr;
                }
                if (v->kind != EKind::Col && (!check_case_types(v, schema) || !check_text(v, schema))) return nullptr;   // a text-valued expression within textsel.hpp's limits
                x->text_num = true;
            }
            // to Utf8 from anything but text (a NULL literal takes the type): the value is formatted (numtext.hpp)
            const int from = expr_static_type(x->l.get(), schema);   // (-1: untyped NULLs alone, or an untyped integer literal)
            x->num_text = x->cast_to == ColType::UTF8 && !ts && from != 4 && (from != -1 || x->l->kind == EKind::LitI);
            return x;
        }
        if (t == "binary_expr") {
            x->kind = EKind::Bin;
            x->s = e->s("op");
            x->l = expr(e->get("left"), schema);
            x->r = expr(e->get("right"), schema);
            return x->l && x->r ? std::move(x) : nullptr;
        }
        if (t == "not_expr" || t == "is_null_expr" || t == "is_not_null_expr" || t == "negative_expr") {
            x->kind = t == "not_expr" ? EKind::Not : t == "is_null_expr" ? EKind::IsNull : t == "is_not_null_expr" ? EKind::IsNotNull : EKind::Neg;
            const JValue *arg = e->get("arg");
            x->l = expr(arg ? arg : e->get("expr"), schema);
            return x->l ? std::move(x) : nullptr;
        }
        if (t == "in_list_expr") {
            x->kind = EKind::InList;
            x->l = expr(e->get("expr"), schema);
            const JValue *list = e->get("list"), *neg = e->get("negated");
            if (!x->l || !list || list->kind != JValue::Arr || list->arr.empty()) { if (x->l) fail("in_list_expr without a list"); return nullptr; }
            x->negated = neg && neg->kind == JValue::Bool && neg->b;
            for (auto &item : list->arr) {
                auto li = expr(item.get(), schema);
                if (!li) return nullptr;
                x->list.push_back(std::move(li));
            }
            return x;
        }
        if (t == "case_expr") {   // CaseExpr { expr: Option, when_then_expr: Vec<(when, then)>, else_expr: Option }
            x->kind = EKind::Case;
            const JValue *base = e->get("expr"), *wt = e->get("when_then_expr"), *el = e->get("else_expr");
            if (!wt || wt->kind != JValue::Arr || wt->arr.empty()) { fail("case_expr without when_then_expr"); return nullptr; }
            if (base && base->kind != JValue::Null && !(x->l = expr(base, schema))) return nullptr;
            if (el && el->kind != JValue::Null && !(x->r = expr(el, schema))) return nullptr;
            for (auto &pair : wt->arr) {
                if (pair->kind != JValue::Arr || pair->arr.size() != 2) { fail("malformed when_then_expr"); return nullptr; }
                auto w = expr(pair->arr[0].get(), schema), th = expr(pair->arr[1].get(), schema);
                if (!w || !th) return nullptr;
                x->list.push_back(std::move(w));
                x->list.push_back(std::move(th));
            }
            return x;
        }
        if (t == "scalar_function_expr") return func(e, schema);
        fail("physical_expr '" + t + "' is not supported");
        return nullptr;
    }

    // scalar_function_expr {name | fun, args, return_type} (valprog.hpp A-F1).  Every refusal starts with the node's tag and names its cause.
    std::unique_ptr<Expr> func(const JValue *e, const std::vector<Field> &schema) {
        auto refuse = [&](const std::string &why) -> std::unique_ptr<Expr> {
            fail("scalar_function_expr: " + why);
            return nullptr;
        };
        auto lower = [](std::string v) {
            for (auto &ch : v) ch = (char)std::tolower((unsigned char)ch);
            return v;
        };
        const JValue *nm = e->get("name");
        if (!nm || nm->kind != JValue::Str) nm = e->get("fun");
        if (!nm || nm->kind != JValue::Str || nm->str.empty()) return refuse("a node without a function name");
        std::string name = lower(nm->str);
        if (name == "character_length" || name == "length") name = "char_length";
        static const std::pair<const char *, Fn> known[] = {{"abs", Fn::Abs}, {"signum", Fn::Signum}, {"floor", Fn::Floor}, {"ceil", Fn::Ceil}, {"round", Fn::Round},
                                                            {"trunc", Fn::Trunc}, {"sqrt", Fn::Sqrt}, {"date_trunc", Fn::DateTrunc}, {"date_part", Fn::DatePart},
                                                            {"octet_length", Fn::OctetLength}, {"char_length", Fn::CharLength}, {"now", Fn::Now},
                                                            {"split_part", Fn::SplitPart}, {"left", Fn::Left}, {"right", Fn::Right}, {"ltrim", Fn::Ltrim},
                                                            {"rtrim", Fn::Rtrim}, {"btrim", Fn::Btrim}};
        const std::pair<const char *, Fn> *k = nullptr;
        for (auto &c : known)
            if (name == c.first) k = &c;
        if (!k) {
            for (const char *f : {"exp", "ln", "log", "log2", "log10", "power", "sin", "cos", "tan", "asin", "acos", "atan"})
                if (name == f) return refuse("function '" + name + "' has no bit-exact counterpart on the device");
            for (const char *f : {"substr", "lower", "upper", "trim", "concat", "concat_ws", "lpad", "rpad", "repeat", "replace",
                                  "reverse", "initcap", "translate", "to_hex", "chr", "md5", "sha256"})
                if (name == f) return refuse("function '" + name + "' produces text: not yet");
            if (name == "starts_with") return refuse("function 'starts_with' yields a Boolean (no Boolean columns at this boundary)");
            return refuse("function '" + name + "' is not supported");
        }
        std::unique_ptr<Expr> x(new Expr());
        x->kind = EKind::Func;
        x->fn = k->second;
        x->s = name;
        x->i = -1;
        const JValue *args = e->get("args");
        std::vector<std::unique_ptr<Expr>> av;
        if (args && args->kind == JValue::Arr)
            for (auto &a : args->arr) {
                auto ax = expr(a.get(), schema);
                if (!ax) return nullptr;
                av.push_back(std::move(ax));
            }
        else if (args && args->kind != JValue::Null) return refuse("function '" + name + "': args is not a list");
        auto static_name = [&](const Expr *a) -> std::string {
            if (expr_is_ts(a) || (a->kind == EKind::Col && schema[(size_t)a->col].is_ts)) return "Timestamp(ms)";
            static const char *names[] = {"Int32", "Int64", "UInt64", "Float64", "Utf8", "Boolean"};
            const int ty = expr_static_type(a, schema);
            return ty >= 0 && ty <= 5 ? names[ty] : ty == -1 ? "an untyped literal" : "no consistent type";
        };
        auto no_utf8_cast = [](const Expr *a) {
            while (a->kind == EKind::Cast && a->cast_to == ColType::UTF8) a = a->l.get();
            return a;
        };
        ColType rt = ColType::F64;
        bool rts = false;
        if (fn_is_math(x->fn)) {
            if (av.size() != 1) return refuse("function '" + name + "' with " + std::to_string(av.size()) + " arguments: it takes one (round(x, n) is not offered)");
            const int ty = expr_static_type(av[0].get(), schema);
            if (ty != 3 || expr_is_ts(av[0].get()))
                return refuse("function '" + name + "': an argument of type " + static_name(av[0].get()) + ((ty >= 0 && ty <= 2) || ty == -1 ? " (an integer argument: the planner casts it to Float64)" : "") +
                              ", it takes Float64");
        } else if (x->fn == Fn::DateTrunc || x->fn == Fn::DatePart) {
            if (av.size() != 2) return refuse("function '" + name + "' with " + std::to_string(av.size()) + " arguments: it takes (unit, timestamp)");
            const Expr *u = no_utf8_cast(av[0].get());
            if (u->kind != EKind::LitS) return refuse("function '" + name + "': the unit argument is not a Utf8 literal");
            static const char *units[] = {"second", "minute", "hour", "day", "week", "month", "year", "dow", "doy"};
            const std::string unit = lower(u->s);
            for (int i = 0; i < 9; ++i)
                if (unit == units[i]) x->i = i;
            const bool trunc = x->fn == Fn::DateTrunc;
            if (x->i < 0 || (trunc && x->i > 6) || (!trunc && x->i == 4))
                return refuse("function '" + name + "': unit '" + u->s + "' (supported: " +
                              (trunc ? "second, minute, hour, day, week, month, year" : "year, month, day, hour, minute, second, dow, doy") + ")");
            const Expr *ts = av[1].get();
            if (!(expr_is_ts(ts) || (ts->kind == EKind::Col && schema[(size_t)ts->col].is_ts)))
                return refuse("function '" + name + "': an argument of type " + static_name(ts) + ", it takes a Timestamp(ms) column or a Timestamp-valued function");
            av.erase(av.begin());
            rt = trunc ? ColType::I64 : ColType::I32;
            rts = trunc;
        } else if (x->fn == Fn::Now) {
            if (!av.empty()) return refuse("function 'now' with " + std::to_string(av.size()) + " arguments: it takes none");
            rt = ColType::I64;
            rts = true;
        } else if (fn_is_slice(x->fn)) {   // textslice.hpp A-SL1..A-SL5
            const bool split = x->fn == Fn::SplitPart, count = x->fn == Fn::Left || x->fn == Fn::Right;
            const std::string who = "function '" + name + "'";
            if (split ? av.size() != 3 : count ? av.size() != 2 : (av.size() != 1 && av.size() != 2))
                return refuse(who + " with " + std::to_string(av.size()) + " arguments: it takes " +
                              (split ? "(string, delimiter, n)" : count ? "(string, n)" : "(string) or (string, characters)"));
            // the value: a Utf8 column or a slice function of one
            // ... and a number or timestamp cast to Utf8 counts as such a column (numtext.hpp A-NT7)
            const Expr *v = av[0].get();
            while (v->kind == EKind::Cast && v->cast_to == ColType::UTF8 && !v->num_text) v = v->l.get();
            const bool inner = v->kind == EKind::Func && fn_is_slice(v->fn);
            if (v->kind == EKind::Cast && v->num_text) {
                if (!check_num_text(v, schema)) return nullptr;
            } else if (!inner && !(v->kind == EKind::Col && schema[(size_t)v->col].type == ColType::UTF8)) {
                const char *what = v->kind == EKind::LitS || v->kind == EKind::LitNull ? "a literal" : v->kind == EKind::Case ? "a CASE" : v->kind == EKind::Col ? "a column that is not Utf8" : "a computed value";
                return refuse(who + ": the value argument is " + what + ", it takes a Utf8 column or a slice function (split_part, left, right, ltrim, rtrim, btrim) of one");
            }
            if (1 + slice_depth(v) > kSliceMaxDepth) return refuse(who + ": slice functions nested more than " + std::to_string(kSliceMaxDepth) + " deep");
            // the others: literals (a cast to the literal's own type may sit in front)
            auto literal = [&](const Expr *a, bool text, const char *arg, const Expr **out) -> bool {
                while (a->kind == EKind::Cast && (text ? a->cast_to == ColType::UTF8 : (a->cast_to == ColType::I32 || a->cast_to == ColType::I64) && !a->cast_ts)) a = a->l.get();
                if (a->kind == EKind::LitNull) { refuse(who + ": a NULL literal as " + arg); return false; }
                if (a->kind != (text ? EKind::LitS : EKind::LitI)) {
                    const bool lit = a->kind == EKind::LitI || a->kind == EKind::LitF || a->kind == EKind::LitS || a->kind == EKind::LitB;
                    refuse(who + ": " + arg + (lit ? std::string(" is not ") + (text ? "a Utf8 literal" : "an integer literal")
                                                   : std::string(" is ") + (a->kind == EKind::Col ? "a column" : "a computed value") + ", it takes a literal"));
                    return false;
                }
                *out = a;
                return true;
            };
            const Expr *lit = nullptr;
            if (split || !count) {
                if (av.size() >= 2) {
                    if (!literal(av[1].get(), true, split ? "the delimiter" : "the characters", &lit)) return nullptr;
                    x->slice_arg = lit->s;
                    x->slice_has_arg = true;
                } else {
                    x->slice_arg = " ";   // the one-argument trims strip U+0020
                }
                if (split && x->slice_arg.empty()) return refuse(who + ": an empty delimiter");
                if (split && x->slice_arg.size() > (size_t)kSliceMaxDelimBytes) return refuse(who + ": a delimiter of more than " + std::to_string(kSliceMaxDelimBytes) + " bytes");
                if (!split) {
                    size_t cps = 0;
                    for (unsigned char ch : x->slice_arg) cps += (ch & 0xc0u) != 0x80u;
                    if (cps > (size_t)kSliceMaxTrimChars) return refuse(who + ": more than " + std::to_string(kSliceMaxTrimChars) + " characters to strip");
                }
            }
            if (split || count) {
                if (!literal(av[split ? 2 : 1].get(), false, "n", &lit)) return nullptr;
                if (lit->big_unsigned || lit->i < INT32_MIN || lit->i > INT32_MAX) return refuse(who + ": n beyond Int32");
                if (split && lit->i <= 0) return refuse(who + ": n = " + std::to_string(lit->i) + ", the field number is positive");
                x->slice_n = lit->i;
            }
            av.resize(1);
            rt = ColType::UTF8;
        } else {
            if (av.size() != 1) return refuse("function '" + name + "' with " + std::to_string(av.size()) + " arguments: it takes one");
            const Expr *c = no_utf8_cast(av[0].get());
            if (c->kind != EKind::Col || schema[(size_t)c->col].type != ColType::UTF8)
                return refuse("function '" + name + "': an argument that is not a Utf8 column (" + (c->kind == EKind::Col ? static_name(c) : std::string("a computed value")) + ")");
            rt = ColType::I32;
        }
        const JValue *rj = e->get("return_type");
        if (rj && rj->kind != JValue::Null) {
            ColType gt;
            bool gts = false;
            Field want;
            want.type = rt;
            want.is_ts = rts;
            if (!parse_type(rj, &gt, &gts) || gt != rt || gts != rts)
                return refuse("function '" + name + "': return_type is not the function's " + type_name(want));
        }
        x->list = std::move(av);
        return x;
    }

    // LIKE / NOT LIKE (strmatch.hpp): a Utf8 column (a cast to Utf8 may sit in front of it) against a literal pattern without a backslash, within the
    // limits of the compiled pattern; `skeleton`: `e` is reached from a filter's predicate through AND / OR / NOT only -- where a leaf of the one-pass
    // predicate program can stand.  Anywhere else (CASE, an operand of a comparison, a projected value) LIKE is refused.
    bool check_like(const Expr *e, const std::vector<Field> &schema, bool skeleton) {
        if (!e) return true;
        const bool like = e->kind == EKind::Bin && (e->s == "Like" || e->s == "NotLike");
        if (like) {
            if (!skeleton) return fail("LIKE inside a computed expression (CASE, an operand, a projected value): it is taken as a filter predicate under AND / OR / NOT only");
            const Expr *c = e->l.get(), *p = e->r.get();
            while (c->kind == EKind::Cast && c->cast_to == ColType::UTF8) c = c->l.get();
            while (p->kind == EKind::Cast && p->cast_to == ColType::UTF8) p = p->l.get();
            if (c->kind != EKind::Col || schema[(size_t)c->col].type != ColType::UTF8) return fail("LIKE on something that is not a Utf8 column");
            if (p->kind != EKind::LitS) return fail("LIKE with a pattern that is not a Utf8 literal");
            if (p->s.find('\\') != std::string::npos) return fail("LIKE pattern with a backslash: there is no escape character");
            int pct = 0;
            for (char ch : p->s) pct += ch == '%';
            if (p->s.size() - (size_t)pct > (size_t)kStrMaxPattern || pct > kStrMaxPieces - 1)
                return fail("LIKE pattern beyond " + std::to_string(kStrMaxPattern) + " bytes / " + std::to_string(kStrMaxPieces - 1) + " '%'");
            return true;
        }
        const bool through = skeleton && (e->kind == EKind::Not || (e->kind == EKind::Bin && (e->s == "And" || e->s == "Or")));
        if (!check_like(e->l.get(), schema, through) || !check_like(e->r.get(), schema, through)) return false;
        for (auto &x : e->list)
            if (!check_like(x.get(), schema, false)) return false;
        return true;
    }

    // CAST(x AS Utf8) of something that is not text (numtext.hpp A-NT1 / A-NT6): x is an Int32 / Int64 / UInt64 / Timestamp(ms) column or expression
    bool check_num_text(const Expr *e, const std::vector<Field> &schema) {
        const std::string who = e->try_cast ? "try_cast_expr: " : "cast_expr: ";
        const Expr *x = e->l.get();
        if (x->kind == EKind::LitI || x->kind == EKind::LitF || x->kind == EKind::LitB)
            return fail(who + "CAST of a literal to Utf8 (a literal operand: write the text itself)");
        const int from = expr_static_type(x, schema);
        if (from == 3) return fail(who + "CAST of a Float64 value to Utf8 (Rust's shortest round-trip form has no counterpart on the device)");
        if (from == 5) return fail(who + "CAST of a Boolean value to Utf8 (no Boolean columns at this boundary)");
        if (from < 0 || from > 2) return fail(who + "CAST to Utf8 of an operand without one numeric type");
        return true;
    }
    // A text-valued expression (textsel.hpp A-T1) in a value position: its sources -- distinct literals and columns -- are collected for the A-T5
    // limits; a branch of another type is refused.
    bool text_sources(const Expr *e, const std::vector<Field> &schema, std::set<std::string> *lits, std::set<int> *cols, std::set<std::string> *slices) {
        switch (e->kind) {
            case EKind::Func: {   // a slice function (textslice.hpp): one source, identical calls once
                if (!fn_is_slice(e->fn)) return fail("CASE branches of different types");
                std::vector<std::string> names;
                for (auto &f : schema) names.push_back(f.name);
                slices->insert(slice_text(e, names));
                return true;
            }
            case EKind::LitS: lits->insert(e->s); return true;
            case EKind::LitNull: return true;
            case EKind::Col:
                if (schema[(size_t)e->col].type != ColType::UTF8) return fail("CASE branches of different types");
                cols->insert(e->col);
                return true;
            case EKind::Cast: {
                if (e->cast_to != ColType::UTF8) return fail("CASE branches of different types");
                if (e->num_text) {   // a number or timestamp made text (numtext.hpp): one column source, identical casts once
                    if (!check_num_text(e, schema)) return false;
                    std::vector<std::string> names;
                    for (auto &f : schema) names.push_back(f.name);
                    slices->insert(expr_text(e, names));
                    return true;
                }
                return text_sources(e->l.get(), schema, lits, cols, slices);
            }
            case EKind::Case:
                for (size_t i = 1; i < e->list.size(); i += 2)
                    if (!text_sources(e->list[i].get(), schema, lits, cols, slices)) return false;
                return !e->r || text_sources(e->r.get(), schema, lits, cols, slices);
            default: return fail("CASE branches of different types");
        }
    }
    // `e` of static type Utf8 is a text-valued expression within the limits of one source table
    bool check_text(const Expr *e, const std::vector<Field> &schema) {
        std::set<std::string> lits;
        std::set<int> cols;
        std::set<std::string> slices;
        if (!text_sources(e, schema, &lits, &cols, &slices)) return false;
        if (lits.size() + cols.size() + slices.size() > (size_t)kTextMaxSources)
            return fail("more than " + std::to_string(kTextMaxSources) + " distinct sources (literals plus columns) in one Utf8-valued expression");
        size_t bytes = 0;
        for (auto &l : lits) bytes += l.size();
        if (bytes > (size_t)kTextMaxLiteralBytes) return fail("more than " + std::to_string(kTextMaxLiteralBytes) + " bytes of literals in one Utf8-valued expression");
        return true;
    }
    // a CASE anywhere in a numeric expression whose branches hold text beside numbers (the static type is the first typed branch's)
    bool check_case_types(const Expr *e, const std::vector<Field> &schema) {
        if (!e) return true;
        if (e->kind == EKind::Case) {
            bool text = false, other = false;
            auto see = [&](const Expr *b) {
                const int t = expr_static_type(b, schema);
                text = text || t == 4;
                other = other || (t >= 0 && t != 4);
            };
            for (size_t i = 1; i < e->list.size(); i += 2) see(e->list[i].get());
            if (e->r) see(e->r.get());
            if (text && other) return fail("CASE branches of different types");
        }
        if (!check_case_types(e->l.get(), schema) || !check_case_types(e->r.get(), schema)) return false;
        for (auto &x : e->list)
            if (!check_case_types(x.get(), schema)) return false;
        return true;
    }

    // An EXPRESSION where an operator reads a column (GROUP BY a % 10, SUM(price * 2), ORDER BY a + b): `in` gets a projection on top (once:
    // `wrapped`) that carries every column through and the expression's value beside them (the general evaluator, valprog.hpp); returns the
    // new column's index in the wrapped schema, -1 when refused (`err` says why).
    int computed_column(std::unique_ptr<Node> &in, bool &wrapped, const JValue *e, const char *what) {
        if (!wrapped) {
            std::unique_ptr<Node> w(new Node());
            w->kind = NKind::Project;
            w->id = plan->n_nodes++;
            w->schema = in->schema;
            for (size_t i = 0; i < in->schema.size(); ++i) {
                std::unique_ptr<Expr> c(new Expr());
                c->kind = EKind::Col;
                c->col = (int)i;
                w->proj.emplace_back(std::move(c), in->schema[i].name);
            }
            w->in.push_back(std::move(in));
            in = std::move(w);
            wrapped = true;
        }
        const std::vector<Field> &below = in->in[0]->schema;
        auto x = expr(e, below);
        if (!x) return -1;
        const int ty = expr_static_type(x.get(), below);
        if (!check_case_types(x.get(), below)) return -1;
        if (ty == 4 && !check_text(x.get(), below)) return -1;   // a text-valued key / argument (textsel.hpp)
        if (ty < 0 || ty > 4) { fail(std::string(what) + " over an expression without a numeric type"); return -1; }
        Field f;
        f.name = "#" + std::to_string(in->schema.size());
        f.type = (ColType)ty;
        f.nullable = true;
        f.is_ts = expr_is_ts(x.get());
        in->proj.emplace_back(std::move(x), f.name);
        in->schema.push_back(f);
        return (int)in->schema.size() - 1;
    }

    static std::string guess_relation(const std::vector<Field> &f) {
        auto has = [&](const char *n) { return std::any_of(f.begin(), f.end(), [&](const Field &x) { return x.name == n; }); };
        if (has("auction") || has("bidder") || has("price")) return "bid";
        if (has("a_id") || has("seller") || has("category")) return "auction";
        if (has("p_id") || has("state") || has("city")) return "person";
        if (has("key") && has("value")) return "side_input";
        if (has("ad_id") || has("event_type")) return "ad_event";
        if (has("c_ad_id") || has("campaign_id")) return "campaign";
        return "";
    }

    std::unique_ptr<Node> node(const JValue *j, int depth = 0) {
        if (!j || j->kind != JValue::Obj || depth > 64) { fail("malformed plan node"); return nullptr; }
        const std::string &t = tag(j);
        // transparent nodes
        if (t == "coalesce_batches_exec" || t == "merge_exec" || t == "coalesce_partitions_exec") return node(j->get("input"), depth + 1);
        std::unique_ptr<Node> n(new Node());
        if (t == "repartition_exec") {
            const JValue *part = j->get("partitioning");
            const JValue *hash = part ? part->get("Hash") : nullptr;
            // HashDiff(exprs, n): the fork's own variant (flock-function/src/aws/window/session.rs:252, global.rs:234; datasource/nexmark/queries/
            // q6.rs:128, q11.rs:168, q12.rs:136): n = COUNT(DISTINCT key), "each partition has a unique key after repartition execution"
            if (!hash && part && part->get("HashDiff")) {
                hash = part->get("HashDiff");
                n->hash_diff = true;
            }
            if (!hash) return node(j->get("input"), depth + 1);  // RoundRobinBatch(n)
            if (hash->kind != JValue::Arr || hash->arr.size() != 2 || hash->arr[0]->kind != JValue::Arr || hash->arr[1]->kind != JValue::Num) {
                fail("malformed Hash partitioning");
                return nullptr;
            }
            n->kind = NKind::Repartition;
            auto in = node(j->get("input"), depth + 1);
            if (!in) return nullptr;
            n->schema = in->schema;
            for (auto &e : hash->arr[0]->arr) {
                if (etag(e.get()) != "column") { fail("Hash partitioning on a computed expression"); return nullptr; }
                const int c = resolve(e.get(), n->schema);
                if (c < 0) { fail("Hash partitioning column not in the schema"); return nullptr; }
                n->hash_cols.push_back(c);
            }
            n->n_parts = (int)hash->arr[1]->inum;
            if (n->hash_cols.empty() || n->n_parts < 1) { fail("Hash partitioning without columns / partitions"); return nullptr; }
            n->in.push_back(std::move(in));
        } else if (t == "memory_exec") {
            n->kind = NKind::Scan;
            std::vector<Field> all;
            if (!fields_of(j->get("schema"), &all)) return nullptr;
            const JValue *proj = j->get("projection");
            if (proj && proj->kind == JValue::Arr && !proj->arr.empty()) {
                bool ok = true;
                for (auto &i : proj->arr) {
                    if (i->kind == JValue::Num && i->inum >= 0 && (size_t)i->inum < all.size()) n->schema.push_back(all[(size_t)i->inum]);
                    else ok = false;
                }
                // fixtures of older fork revisions list only the projected fields: indices then exceed the list
                if (!ok) n->schema = all;
            } else {
                n->schema = all;
            }
            Leaf lf;
            lf.schema = n->schema;
            lf.relation = guess_relation(lf.schema);
            n->leaf = (int)plan->leaves.size();
            plan->leaves.push_back(lf);
        } else if (t == "filter_exec") {
            n->kind = NKind::Filter;
            auto in = node(j->get("input"), depth + 1);
            if (!in) return nullptr;
            n->schema = in->schema;
            n->pred = expr(j->get("predicate"), n->schema);
            if (!n->pred || !check_like(n->pred.get(), n->schema, true)) return nullptr;
            n->in.push_back(std::move(in));
        } else if (t == "projection_exec") {
            n->kind = NKind::Project;
            auto in = node(j->get("input"), depth + 1);
            if (!in) return nullptr;
            const JValue *ex = j->get("expr");
            if (!ex || ex->kind != JValue::Arr) { fail("projection_exec without expr"); return nullptr; }
            for (auto &pair : ex->arr) {
                if (pair->kind != JValue::Arr || pair->arr.size() < 2 || pair->arr[1]->kind != JValue::Str) { fail("malformed projection expr"); return nullptr; }
                auto e = expr(pair->arr[0].get(), in->schema);
                if (!e) return nullptr;
                Field f;
                f.name = pair->arr[1]->str;
                if (e->kind == EKind::Col) {
                    const Field &src = in->schema[(size_t)e->col];
                    f.type = src.type; f.is_ts = src.is_ts; f.nullable = src.nullable;
                } else {   // computed: q1's `literal * column` kernel or the general evaluator (valprog.hpp) for a numeric result, textsel.hpp for text
                    const int ty = expr_static_type(e.get(), in->schema);
                    if (!check_case_types(e.get(), in->schema)) return nullptr;
                    if (ty == 4 && !check_text(e.get(), in->schema)) return nullptr;
                    if (ty < 0 || ty > 4) { fail(ty == 5 ? "projection of a Boolean expression (no Boolean columns at this boundary)" : "projection expression without a numeric type"); return nullptr; }
                    if (!check_like(e.get(), in->schema, false)) return nullptr;
                    f.type = (ColType)ty;
                    f.nullable = true;
                    f.is_ts = expr_is_ts(e.get());   // CAST(x AS Timestamp(Millisecond)), date_trunc, now()
                }
                n->proj.emplace_back(std::move(e), f.name);
                n->schema.push_back(f);
            }
            n->in.push_back(std::move(in));
        } else if (t == "hash_aggregate_exec") {
            n->kind = NKind::Aggregate;
            if (!parse_agg_mode(j->s("mode"), &n->mode)) { fail("aggregate mode '" + j->s("mode") + "'"); return nullptr; }
            // COUNT(DISTINCT) (distinct.hpp A-D5): its Partial state is a List column.  Final / FinalPartitioned over the Partial of the same plan --
            // identical group and aggregate lists, only repartitions / coalesces between -- is read as ONE aggregation over the Partial's input:
            // `src` = the Partial, whose entries carry the argument expressions.  Any other Partial with a distinct count is refused.
            const bool distinct = json_has_distinct_count(j);
            const JValue *src = j;
            if (distinct && n->mode == AggMode::Partial) {
                fail("distinct_count in a Partial aggregate that is not read by the Final of the same plan: its partial state is a List column, and there is no list state at this boundary");
                return nullptr;
            }
            if (distinct) {
                src = partial_below(j);
                n->single_pass = src != nullptr;
                if (!src) src = j;
            }
            auto in = node(src->get("input"), depth + 1);
            if (!in) return nullptr;
            if (distinct && !n->single_pass) {
                fail("distinct_count in a " + std::string(agg_mode_name(n->mode)) + " aggregate that is not over the Partial of the same plan: there is no list state at this boundary");
                return nullptr;
            }
            const bool is_final = n->mode != AggMode::Partial && !n->single_pass;
            const JValue *names = j->get("group_expr");   // (single pass: the upper node names the key columns)
            // A group key or an aggregate argument that is an EXPRESSION (GROUP BY a % 10, SUM(price * 2)): the stage that evaluates it
            // (Partial) gets a projection underneath that carries every input column through and the expression's value beside them
            // (the general evaluator, valprog.hpp); the aggregate then reads a column, as ever.  -1: refused (plan->why says why).
            bool wrapped = false;
            auto computed = [&](const JValue *e, const char *what) -> int { return computed_column(in, wrapped, e, what); };
            const JValue *ge = src->get("group_expr");
            size_t gi = 0;
            if (ge && ge->kind == JValue::Arr)
                for (auto &pair : ge->arr) {
                    if (pair->kind != JValue::Arr || pair->arr.size() < 2) { fail("malformed group_expr"); return nullptr; }
                    // the final stage reads the group keys by POSITION from the partial stage's output
                    // (DataFusion's merge expressions); the partial / single stage evaluates the expression
                    int c = -1;
                    if (is_final && gi < in->schema.size()) c = (int)gi;
                    else if (etag(pair->arr[0].get()) == "column") c = resolve(pair->arr[0].get(), in->schema);
                    else if (!is_final) c = computed(pair->arr[0].get(), "GROUP BY");
                    if (c < 0) { fail("GROUP BY on something that is neither an input column nor a numeric expression"); return nullptr; }
                    n->group.push_back(c);
                    Field f = in->schema[(size_t)c];
                    f.name = pair->arr[1]->kind == JValue::Str ? pair->arr[1]->str : f.name;
                    if (n->single_pass && names->arr[gi]->kind == JValue::Arr && names->arr[gi]->arr.size() >= 2 && names->arr[gi]->arr[1]->kind == JValue::Str)
                        f.name = names->arr[gi]->arr[1]->str;
                    n->schema.push_back(f);
                    ++gi;
                }
            const JValue *ae = src->get("aggr_expr");
            int state_at = (int)n->group.size();  // Final: position of the next aggregate's first state column
            int n_distinct = 0;
            if (ae && ae->kind == JValue::Arr)
                for (auto &x : ae->arr) {
                    Agg a;
                    a.name = x->s("name");
                    bool ts = false;
                    const bool dc = is_distinct_count_tag(x->s("aggregate_expr"));
                    if (!parse_type(x->get("data_type"), &a.type, &ts) && !(dc && !x->get("data_type"))) { fail("aggregate '" + a.name + "' of an unsupported type"); return nullptr; }
                    if (dc) {
                        a.fn = AggFn::CountDistinct;
                        if (++n_distinct > kMaxDistinctCounts) { fail("more than " + std::to_string(kMaxDistinctCounts) + " distinct counts in one aggregate (each owns a table)"); return nullptr; }
                    } else if (!parse_agg_fn(x->s("aggregate_expr"), &a.fn)) {
                        fail("aggregate function '" + x->s("aggregate_expr") + "' (supported: count, max, min, sum, avg, distinct_count)");
                        return nullptr;
                    }
                    const std::string fn = agg_fn_name(a.fn);
                    if (is_final) {
                        a.arg = state_at;  // state columns, by position
                        if (a.fn == AggFn::Avg) a.arg2 = state_at + 1;
                        state_at += agg_state_cols(a.fn);
                        if ((size_t)state_at > in->schema.size()) { fail("final aggregate without its state column"); return nullptr; }
                    } else {
                        const JValue *arg = x->get("expr");
                        const JValue *args = dc ? x->get("exprs") : nullptr;   // (the fork's tag cannot be checked: the argument under `exprs`, a list of one, or `expr`)
                        if (args && args->kind == JValue::Arr) {
                            if (args->arr.size() != 1) { fail("distinct_count over " + std::to_string(args->arr.size()) + " argument expressions: it takes one"); return nullptr; }
                            arg = args->arr[0].get();
                        }
                        if (arg && etag(arg) == "column") {
                            a.arg = resolve(arg, in->schema);
                            if (a.arg < 0) { fail("aggregate argument not in the input schema"); return nullptr; }
                        } else if (arg && etag(arg) != "literal") {   // SUM(price * 2), COUNT(CASE ...): the expression becomes a column underneath
                            a.arg = computed(arg, ("aggregate '" + fn + "'").c_str());
                            if (a.arg < 0) return nullptr;
                        } else if (a.fn != AggFn::Count) {
                            fail("aggregate '" + fn + "' over a literal");
                            return nullptr;
                        }
                    }
                    if (dc && !agg_takes(a.fn, in->schema[(size_t)a.arg].type)) { fail("distinct_count needs an integer or Utf8 column"); return nullptr; }
                    if (a.fn == AggFn::Count || dc) a.type = ColType::U64;
                    if (a.fn == AggFn::Avg) a.type = ColType::F64;
                    Field f;
                    f.nullable = true;
                    f.is_ts = ts && agg_is_minmax(a.fn);   // MIN / MAX of a Timestamp column is a Timestamp (q11's start_time / end_time)
                    if (is_final || n->single_pass) {
                        f.name = a.name;
                        f.type = a.type;
                        n->schema.push_back(f);
                    } else if (a.fn == AggFn::Avg) {
                        f.name = a.name + "[count]";
                        f.type = ColType::U64;
                        n->schema.push_back(f);
                        f.name = a.name + "[sum]";
                        f.type = ColType::F64;
                        n->schema.push_back(f);
                    } else {
                        f.name = a.name + "[" + fn + "]";
                        f.type = a.type;
                        n->schema.push_back(f);
                    }
                    n->aggs.push_back(a);
                }
            // no GROUP BY (reduce.hpp): the argument types of agg_takes, less COUNT of a Utf8 column (the pass streams fixed-width columns); up to eight
            // accumulators (AVG takes two)
            if (n->group.empty()) {
                int accs = 0;
                for (auto &a : n->aggs) {
                    accs += agg_accumulators(a.fn);
                    if (a.arg < 0 || a.fn == AggFn::CountDistinct) continue;
                    const ColType at = in->schema[(size_t)a.arg].type;
                    if (!agg_takes(a.fn, at) || at == ColType::UTF8) { fail(std::string(agg_fn_name(a.fn)) + " needs an integer column"); return nullptr; }
                }
                if (accs > kMaxUngroupedAccumulators) { fail("more than " + std::to_string(kMaxUngroupedAccumulators) + " accumulators in one ungrouped aggregate"); return nullptr; }
            } else {   // GROUP BY: up to four in the tables of relops.hpp, five to sixteen in the one pass over group ids of groupwide.hpp
                int accs = 0;
                for (auto &a : n->aggs) accs += agg_accumulators(a.fn);
                if (accs > kMaxGroupedAccumulators) { fail("more than " + std::to_string(kMaxGroupedAccumulators) + " accumulators in one GROUP BY"); return nullptr; }
            }
            n->in.push_back(std::move(in));
        } else if (t == "hash_join_exec") {
            n->kind = NKind::Join;
            const std::string jt = j->s("join_type");
            if (jt == "Semi") n->join_type = JoinType::Semi;
            else if (jt == "Anti") n->join_type = JoinType::Anti;
            else if (jt != "Inner") { fail("join_type '" + jt + "': only Inner, Semi and Anti joins"); return nullptr; }
            const bool semi = n->join_type != JoinType::Inner;
            n->join_partitioned = j->s("mode") == "Partitioned";
            auto l = node(j->get("left"), depth + 1);
            if (!l) return nullptr;
            auto r = node(j->get("right"), depth + 1);
            if (!r) return nullptr;
            const JValue *on = j->get("on");
            if (!on || on->kind != JValue::Arr || on->arr.empty() || on->arr.size() > (size_t)kMaxJoinPairs) {
                fail("join on no key pair or on more than 8 key pairs");
                return nullptr;
            }
            for (auto &pair : on->arr)
                if (pair->kind != JValue::Arr || pair->arr.size() != 2) { fail("malformed join key pair"); return nullptr; }
            auto keycol = [&](const JValue *k, const std::vector<Field> &schema) {
                if (k->kind == JValue::Str) {  // older fork revision: bare names
                    for (size_t i = 0; i < schema.size(); ++i)
                        if (schema[i].name == k->str) return (int)i;
                    return -1;
                }
                return resolve(k, schema);
            };
            for (auto &pair : on->arr) {
                n->on.push_back(KeyPair{keycol(pair->arr[0].get(), l->schema), keycol(pair->arr[1].get(), r->schema)});
                if (n->on.back().l < 0 || n->on.back().r < 0) { fail("join key not in the input schemas"); return nullptr; }
            }
            n->schema = l->schema;
            if (!semi) n->schema.insert(n->schema.end(), r->schema.begin(), r->schema.end());
            if (semi) {
                // Semi / Anti (relops.hpp A-S2): the left input's schema.  A serialised schema that says otherwise -- right columns carried along, other
                // types -- is another operator's; key pairs that cannot compare are refused here, in the words the inner join's execute uses
                const char *kind = n->join_type == JoinType::Semi ? "Semi" : "Anti";
                const JValue *sc = j->get("schema");
                const JValue *sf = sc ? sc->get("fields") : nullptr;
                if (sf && sf->kind == JValue::Arr) {
                    std::vector<Field> given;
                    if (!fields_of(sc, &given)) return nullptr;
                    bool same = given.size() == l->schema.size();
                    for (size_t i = 0; same && i < given.size(); ++i) same = given[i].type == l->schema[i].type && given[i].is_ts == l->schema[i].is_ts;
                    if (!same) {
                        fail(std::string(kind) + " join: the node's schema (" + std::to_string(given.size()) + " columns) is not the left input's (" +
                             std::to_string(l->schema.size()) + " columns): a " + kind + " join returns left columns only");
                        return nullptr;
                    }
                }
                bool ok = true;
                for (auto &k : n->on) ok = ok && join_keys_comparable(l->schema[(size_t)k.l].type, r->schema[(size_t)k.r].type);
                if (!ok) { fail(std::string(kind) + " join: join keys must be integer columns of one signedness, or two Utf8 columns"); return nullptr; }
            }
            n->in.push_back(std::move(l));
            n->in.push_back(std::move(r));
        } else if (t == "cross_join_exec") {
            // CrossJoinExec (cross.hpp): `left`, `right`, optionally `schema`; `on`, `join_type`, `mode`, `random_state`, where present, are ignored
            n->kind = NKind::Join;
            n->join_type = JoinType::Cross;
            auto l = node(j->get("left"), depth + 1);
            if (!l) return nullptr;
            auto r = node(j->get("right"), depth + 1);
            if (!r) return nullptr;
            n->schema = l->schema;
            n->schema.insert(n->schema.end(), r->schema.begin(), r->schema.end());
            // (A-X1) a serialised schema that is not left ++ right -- a column short, another type -- is another operator's
            const JValue *sc = j->get("schema");
            const JValue *sf = sc ? sc->get("fields") : nullptr;
            if (sf && sf->kind == JValue::Arr) {
                std::vector<Field> given;
                if (!fields_of(sc, &given)) return nullptr;
                if (given.size() != n->schema.size()) {
                    fail("Cross join: the node's schema (" + std::to_string(given.size()) + " columns) is not the left input's followed by the right input's (" +
                         std::to_string(l->schema.size()) + " + " + std::to_string(r->schema.size()) + " columns)");
                    return nullptr;
                }
                for (size_t i = 0; i < given.size(); ++i)
                    if (given[i].type != n->schema[i].type || given[i].is_ts != n->schema[i].is_ts) {
                        fail("Cross join: the node's schema says " + std::string(type_name(given[i])) + " for column " + std::to_string(i) + " ('" + given[i].name +
                             "'), the inputs give " + type_name(n->schema[i]) + ": a cross join returns left ++ right columns unchanged");
                        return nullptr;
                    }
            }
            n->in.push_back(std::move(l));
            n->in.push_back(std::move(r));
        } else if (t == "union_exec") {
            // UnionExec (union.hpp): `inputs`, optionally `schema`.  A union that arrives as an input -- node() has already looked through the
            // transparent nodes above it -- gives its inputs to this one
            n->kind = NKind::Union;
            plan->has_union = true;
            const JValue *ins = j->get("inputs");
            if (!ins || ins->kind != JValue::Arr || ins->arr.empty()) { fail("Union: no inputs (union_exec takes `inputs`, a list of at least one plan)"); return nullptr; }
            for (auto &x : ins->arr) {
                auto c = node(x.get(), depth + 1);
                if (!c) return nullptr;
                if (c->kind == NKind::Union) {
                    for (auto &g : c->in) n->in.push_back(std::move(g));
                } else {
                    n->in.push_back(std::move(c));
                }
                if (n->in.size() > (size_t)kMaxUnionInputs) {
                    fail("Union: more than " + std::to_string(kMaxUnionInputs) + " inputs after flattening (at least " + std::to_string(n->in.size()) + ")");
                    return nullptr;
                }
            }
            // (A-U1) names from input 0; every input its column count, types and is_ts; nullable when any input's column is
            n->schema = n->in[0]->schema;
            for (size_t k = 1; k < n->in.size(); ++k) {
                const std::vector<Field> &sk = n->in[k]->schema;
                if (sk.size() != n->schema.size()) {
                    fail("Union: input " + std::to_string(k) + " has " + std::to_string(sk.size()) + " columns, input 0 has " + std::to_string(n->schema.size()));
                    return nullptr;
                }
                for (size_t i = 0; i < sk.size(); ++i) {
                    if (sk[i].type != n->schema[i].type || sk[i].is_ts != n->schema[i].is_ts) {
                        fail("Union: input " + std::to_string(k) + " gives " + type_name(sk[i]) + " for column " + std::to_string(i) + " ('" + sk[i].name + "'), input 0 gives " +
                             type_name(n->schema[i]) + " ('" + n->schema[i].name + "'): the inputs of a union have one schema");
                        return nullptr;
                    }
                    n->schema[i].nullable = n->schema[i].nullable || sk[i].nullable;
                }
            }
            const JValue *sc = j->get("schema");
            const JValue *sf = sc ? sc->get("fields") : nullptr;
            if (sf && sf->kind == JValue::Arr) {
                std::vector<Field> given;
                if (!fields_of(sc, &given)) return nullptr;
                if (given.size() != n->schema.size()) {
                    fail("Union: the node's schema (" + std::to_string(given.size()) + " columns) is not its inputs' (" + std::to_string(n->schema.size()) + " columns)");
                    return nullptr;
                }
                for (size_t i = 0; i < given.size(); ++i)
                    if (given[i].type != n->schema[i].type || given[i].is_ts != n->schema[i].is_ts) {
                        fail("Union: the node's schema says " + std::string(type_name(given[i])) + " for column " + std::to_string(i) + " ('" + given[i].name +
                             "'), the inputs give " + type_name(n->schema[i]) + ": a union returns its inputs' columns unchanged");
                        return nullptr;
                    }
            }
        } else if (t == "sort_exec") {
            n->kind = NKind::Sort;
            auto in = node(j->get("input"), depth + 1);
            if (!in) return nullptr;
            const size_t n_in = in->schema.size();
            bool wrapped = false;
            const JValue *ex = j->get("expr");
            if (!ex || ex->kind != JValue::Arr || ex->arr.empty()) { fail("sort_exec without expr"); return nullptr; }
            for (auto &k : ex->arr) {
                const JValue *e = k->get("expr");
                if (!e) { fail("sort_exec key without expr"); return nullptr; }
                SortCol sc;
                // ORDER BY an expression: its value becomes a column underneath (computed_column) and is dropped again above the sort
                sc.col = etag(e) == "column" ? resolve(e, in->schema) : computed_column(in, wrapped, e, "ORDER BY");
                if (sc.col < 0) { if (err.empty()) fail("ORDER BY column '" + e->s("name") + "' not in the input schema"); return nullptr; }
                const JValue *opt = k->get("options");
                const JValue *d = opt ? opt->get("descending") : nullptr, *nf = opt ? opt->get("nulls_first") : nullptr;
                sc.descending = d && d->kind == JValue::Bool && d->b;
                sc.nulls_first = nf && nf->kind == JValue::Bool && nf->b;
                n->sort_cols.push_back(sc);
            }
            n->schema = in->schema;
            n->in.push_back(std::move(in));
            if (wrapped) {   // the sort's own columns only: a projection on top takes the computed keys out again
                n->id = plan->n_nodes++;
                std::unique_ptr<Node> top(new Node());
                top->kind = NKind::Project;
                for (size_t i = 0; i < n_in; ++i) {
                    std::unique_ptr<Expr> c(new Expr());
                    c->kind = EKind::Col;
                    c->col = (int)i;
                    top->proj.emplace_back(std::move(c), n->schema[i].name);
                    top->schema.push_back(n->schema[i]);
                }
                top->in.push_back(std::move(n));
                n = std::move(top);
            }
        } else if (t == "window_agg_exec") {
            // WindowAggExec (q6.sql: ROW_NUMBER() OVER (PARTITION BY a_id ORDER BY price DESC), benchmarks/src/nexmark/query/q6_plan.fmt:6,11).
            // The physical planner sorts the input by (PARTITION BY, ORDER BY) underneath (a sort_exec); the operator numbers the rows of every
            // RUN of equal partition keys 1, 2, ... in the order they arrive -- what DataFusion's partition points over a sorted batch give.
            // Output: the window columns first, then the input's (q6_plan.fmt's schemas).  ROW_NUMBER() and the aggregates COUNT / SUM / MIN / MAX /
            // AVG ("window_expr": "aggregate_window_expr", DataFusion's AggregateWindowExpr) over the default frame are taken.
            n->kind = NKind::Window;
            auto in = node(j->get("input"), depth + 1);
            if (!in) return nullptr;
            const JValue *we = j->get("window_expr");
            if (!we || we->kind != JValue::Arr || we->arr.empty()) { fail("window_agg_exec without window_expr"); return nullptr; }
            std::vector<Field> wf;
            auto key_col = [&](const JValue *e, const char *what) -> int {
                if (etag(e) != "column") { fail(std::string(what) + " on something other than a column"); return -1; }
                const int c = resolve(e, in->schema);
                if (c < 0) { fail(std::string(what) + " column not in the input schema"); return -1; }
                return c;
            };
            for (auto &w : we->arr) {
                if (w->kind != JValue::Obj) { fail("malformed window_expr"); return nullptr; }
                WinExpr x;
                Field f;
                f.nullable = true;
                const JValue *ag = w->get("aggregate");
                if (w->s("window_expr") == "aggregate_window_expr" || (ag && ag->kind == JValue::Obj)) {
                    if (!ag || ag->kind != JValue::Obj) { fail("aggregate_window_expr without its aggregate"); return nullptr; }
                    x.row_number = false;
                    std::string fn = ag->s("aggregate_expr");
                    for (auto &ch : fn) ch = (char)std::tolower((unsigned char)ch);
                    if (!parse_agg_fn(fn, &x.fn)) {
                        fail("window function '" + fn + "' (supported: ROW_NUMBER, COUNT, SUM, MIN, MAX, AVG)");
                        return nullptr;
                    }
                    f.name = ag->s("name");
                    if (!parse_type(ag->get("data_type"), &x.type, &x.is_ts)) { fail("window aggregate '" + f.name + "' of an unsupported type"); return nullptr; }
                    const JValue *arg = ag->get("expr");
                    if (arg && etag(arg) == "column") {
                        x.arg = resolve(arg, in->schema);
                        if (x.arg < 0) { fail("window aggregate argument not in the input schema"); return nullptr; }
                    } else if (arg && etag(arg) != "literal") {
                        fail("window aggregate '" + fn + "' over a computed expression");
                        return nullptr;
                    } else if (x.fn != AggFn::Count) {
                        fail("window aggregate '" + fn + "' over a literal");
                        return nullptr;
                    }
                    const ColType at = x.arg >= 0 ? in->schema[(size_t)x.arg].type : ColType::U64;
                    if (!agg_takes(x.fn, at)) {
                        fail(fn + " needs an integer column");
                        return nullptr;
                    }
                    if (x.fn == AggFn::Count) x.type = ColType::U64;
                    if (x.fn == AggFn::Avg) x.type = ColType::F64;
                    x.is_ts = x.is_ts && agg_is_minmax(x.fn);
                    if (agg_is_minmax(x.fn) && (x.type == ColType::F64) != (at == ColType::F64)) {
                        fail(fn + " of a column into a column of another kind");
                        return nullptr;
                    }
                    if (x.type == ColType::UTF8) { fail("window aggregate '" + f.name + "' of an unsupported type"); return nullptr; }
                    const JValue *ob = w->get("order_by");
                    if (ob && ob->kind == JValue::Arr)
                        for (auto &e : ob->arr) {
                            SortCol sc;
                            const JValue *ex = e->kind == JValue::Obj && e->get("expr") ? e->get("expr") : e.get();
                            sc.col = key_col(ex, "ORDER BY");
                            if (sc.col < 0) return nullptr;
                            const JValue *op = e->get("options");
                            if (op && op->get("descending") && op->get("descending")->kind == JValue::Bool) sc.descending = op->get("descending")->b;
                            if (op && op->get("nulls_first") && op->get("nulls_first")->kind == JValue::Bool) sc.nulls_first = op->get("nulls_first")->b;
                            x.order.push_back(sc);
                        }
                    // the frame: absent, null, or exactly the default (RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW)
                    const JValue *fr = w->get("window_frame");
                    if (fr && fr->kind != JValue::Null) {
                        auto bound = [](const JValue *b) -> std::string {   // "Preceding(None)" | "CurrentRow" | "Following(3)" ...
                            if (!b) return "?";
                            if (b->kind == JValue::Str) return b->str;
                            if (b->kind == JValue::Obj && b->obj.size() == 1) {
                                const JValue *v = b->obj[0].second.get();
                                return b->obj[0].first + "(" + (v->kind == JValue::Null ? std::string("None") : v->kind == JValue::Num ? std::to_string(v->inum) : std::string("?")) + ")";
                            }
                            return "?";
                        };
                        const std::string units = fr->kind == JValue::Obj ? fr->s("units") : std::string("?"),
                                          lo = fr->kind == JValue::Obj ? bound(fr->get("start_bound")) : "?", hi = fr->kind == JValue::Obj ? bound(fr->get("end_bound")) : "?";
                        const bool dflt = (units == "Range" || units == "RANGE") && (lo == "Preceding(None)" || lo == "UnboundedPreceding") &&
                                          (hi == "CurrentRow" || hi == "CurrentRow(None)");
                        if (!dflt) {
                            fail("window frame " + units + " BETWEEN " + lo + " AND " + hi + " (supported: the default RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW)");
                            return nullptr;
                        }
                    }
                    f.type = x.type;
                    f.is_ts = x.is_ts;
                    if (f.name.empty()) f.name = w->s("name");
                } else {
                    std::string fun;
                    for (const char *key : {"fun", "function", "window_function", "built_in", "expr", "name"}) {
                        const JValue *fv = w->get(key);
                        if (!fv) continue;
                        std::string v = fv->kind == JValue::Str ? fv->str : (fv->kind == JValue::Obj && !fv->obj.empty() ? fv->obj[0].first : std::string());
                        for (auto &ch : v) ch = (char)std::tolower((unsigned char)ch);
                        v.erase(std::remove(v.begin(), v.end(), '_'), v.end());
                        if (v.find("rownumber") != std::string::npos) { fun = "row_number"; break; }
                        if (fun.empty() && !v.empty()) fun = v;
                    }
                    if (fun != "row_number") { fail("window function '" + fun + "' (supported: ROW_NUMBER, COUNT, SUM, MIN, MAX, AVG)"); return nullptr; }
                    const JValue *nm = w->get("name");
                    f.name = nm && nm->kind == JValue::Str ? nm->str : "ROW_NUMBER()";
                    f.type = ColType::U64;
                }
                const JValue *pb = w->get("partition_by");
                if (pb && pb->kind == JValue::Arr)
                    for (auto &e : pb->arr) {
                        const int c = key_col(e.get(), "PARTITION BY");
                        if (c < 0) return nullptr;
                        x.part.push_back(c);
                    }
                if (!x.row_number) {   // (ROW_NUMBER keeps its execute-time checks)
                    if (x.part.size() > (size_t)kMaxWindowKeys) { fail("PARTITION BY more than four columns"); return nullptr; }
                    if (x.order.size() > (size_t)kMaxWindowKeys) { fail("window ORDER BY more than four columns"); return nullptr; }
                    for (int c : x.part)
                        if (in->schema[(size_t)c].type == ColType::UTF8) { fail("PARTITION BY a Utf8 column"); return nullptr; }
                    for (auto &o : x.order)
                        if (in->schema[(size_t)o.col].type == ColType::UTF8) { fail("window ORDER BY a Utf8 column"); return nullptr; }
                }
                n->win.push_back(x);
                wf.push_back(f);
            }
            n->schema = wf;
            n->schema.insert(n->schema.end(), in->schema.begin(), in->schema.end());
            n->in.push_back(std::move(in));
        } else if (t == "global_limit_exec" || t == "local_limit_exec") {
            n->kind = NKind::Limit;
            auto in = node(j->get("input"), depth + 1);
            if (!in) return nullptr;
            n->schema = in->schema;
            const JValue *l = j->get("limit");
            if (!l || l->kind != JValue::Num || !l->is_int || l->inum < 0) { fail("limit without a row count"); return nullptr; }
            n->limit = l->inum;
            n->in.push_back(std::move(in));
        } else {
            fail("execution_plan '" + t + "' is not supported");
            return nullptr;
        }
        n->id = plan->n_nodes++;
        return n;
    }
};

inline void expr_cols(const Expr *e, std::set<int> *out) {
    if (!e) return;
    if (e->kind == EKind::Col) out->insert(e->col);
    expr_cols(e->l.get(), out);
    expr_cols(e->r.get(), out);
    for (auto &li : e->list) expr_cols(li.get(), out);
}

// Marks, top-down, the output columns of every node that something above it reads; leaves learn which of their
// columns have to reach the device at all.
inline void mark_required(Plan *p, Node *n, const std::vector<char> &req) {
    n->required = req;
    auto need = [](std::vector<char> &v, int c) { if (c >= 0 && (size_t)c < v.size()) v[(size_t)c] = 1; };
    switch (n->kind) {
        case NKind::Scan: {
            Leaf &lf = p->leaves[(size_t)n->leaf];
            if (lf.needed.size() != n->schema.size()) lf.needed.assign(n->schema.size(), 0);
            for (size_t i = 0; i < req.size(); ++i) lf.needed[i] |= req[i];
            break;
        }
        case NKind::Filter: {
            std::vector<char> r = req;
            std::set<int> cs;
            expr_cols(n->pred.get(), &cs);
            for (int c : cs) need(r, c);
            mark_required(p, n->in[0].get(), r);
            break;
        }
        case NKind::Project: {
            std::vector<char> r(n->in[0]->schema.size(), 0);
            for (size_t i = 0; i < n->proj.size(); ++i)
                if (req[i]) {
                    std::set<int> cs;
                    expr_cols(n->proj[i].first.get(), &cs);
                    for (int c : cs) need(r, c);
                }
            mark_required(p, n->in[0].get(), r);
            break;
        }
        case NKind::Aggregate: {
            std::vector<char> r(n->in[0]->schema.size(), 0);
            for (int c : n->group) need(r, c);
            for (auto &a : n->aggs) { need(r, a.arg); need(r, a.arg2); }
            mark_required(p, n->in[0].get(), r);
            break;
        }
        case NKind::Join: {
            const size_t nl = n->in[0]->schema.size();
            // (Semi / Anti: the output IS the left side; the right child is read for its key columns alone -- a leaf under it uploads nothing else)
            // (Cross: no keys -- each side gets what the ancestors read of it, COUNT(*) above asks neither side for a column)
            const bool semi = n->join_type == JoinType::Semi || n->join_type == JoinType::Anti;
            std::vector<char> l(req.begin(), req.begin() + nl), r;
            if (semi) r.assign(n->in[1]->schema.size(), 0);
            else r.assign(req.begin() + nl, req.end());
            for (auto &k : n->on) { need(l, k.l); need(r, k.r); }
            mark_required(p, n->in[0].get(), l);
            mark_required(p, n->in[1].get(), r);
            break;
        }
        case NKind::Repartition: {
            std::vector<char> r = req;
            for (int c : n->hash_cols) need(r, c);
            mark_required(p, n->in[0].get(), r);
            break;
        }
        case NKind::Sort: {
            std::vector<char> r = req;
            for (auto &k : n->sort_cols) need(r, k.col);
            mark_required(p, n->in[0].get(), r);
            break;
        }
        case NKind::Limit:
            mark_required(p, n->in[0].get(), req);
            break;
        case NKind::Window: {
            const size_t nw = n->win.size();
            std::vector<char> r(req.begin() + (long)nw, req.end());
            for (auto &x : n->win) {
                for (int c : x.part) need(r, c);
                for (auto &o : x.order) need(r, o.col);
                need(r, x.arg);
            }
            mark_required(p, n->in[0].get(), r);
            break;
        }
        case NKind::Union:   // output column c is column c of every input
            for (auto &c : n->in) mark_required(p, c.get(), req);
            break;
    }
}

// The columns whose NULL makes `e` NULL: reached through arithmetic, comparisons, casts, unary minus and scalar functions only.  A column under CASE, IS [NOT] NULL,
// IN, NOT, AND / OR does not count -- `CASE WHEN f <= f THEN 100 ELSE i END` has a value where f is NULL.
inline void strict_cols(const Expr *e, std::set<int> *out) {
    if (!e) return;
    switch (e->kind) {
        case EKind::Col: out->insert(e->col); return;
        case EKind::Cast: case EKind::Neg: strict_cols(e->l.get(), out); return;
        case EKind::Func:   // a function of a NULL is NULL (A-F2)
            for (auto &a : e->list) strict_cols(a.get(), out);
            return;
        case EKind::Bin:
            if (e->s == "And" || e->s == "Or") return;
            strict_cols(e->l.get(), out);
            strict_cols(e->r.get(), out);
            return;
        default: return;
    }
}

// droppable[c]: dropping the rows of `n`'s output whose column c is NULL leaves the plan's result unchanged.
inline void mark_null_droppable(Plan *p, const Node *n, const std::vector<char> &droppable) {
    switch (n->kind) {
        case NKind::Scan: {
            Leaf &lf = p->leaves[(size_t)n->leaf];
            if (lf.null_droppable.size() != n->schema.size()) lf.null_droppable.assign(n->schema.size(), 1);
            for (size_t i = 0; i < droppable.size(); ++i) lf.null_droppable[i] &= droppable[i];
            break;
        }
        case NKind::Filter: {
            std::vector<char> d = droppable;
            // comparisons with NULL are NULL, and a NULL predicate drops the row -- through AND, not through OR
            std::vector<const Expr *> stack{n->pred.get()};
            while (!stack.empty()) {
                const Expr *e = stack.back();
                stack.pop_back();
                if (e->kind == EKind::Bin && e->s == "And") { stack.push_back(e->l.get()); stack.push_back(e->r.get()); continue; }
                if (e->kind == EKind::Bin && e->s != "Or") {
                    std::set<int> cs;
                    strict_cols(e, &cs);
                    for (int c : cs) d[(size_t)c] = 1;
                }
            }
            mark_null_droppable(p, n->in[0].get(), d);
            break;
        }
        case NKind::Project: {
            std::vector<char> d(n->in[0]->schema.size(), 0);
            for (size_t i = 0; i < n->proj.size(); ++i)
                if (droppable[i] && n->proj[i].first->kind == EKind::Col) d[(size_t)n->proj[i].first->col] = 1;
            mark_null_droppable(p, n->in[0].get(), d);
            break;
        }
        case NKind::Aggregate: {
            std::vector<char> d(n->in[0]->schema.size(), 0);
            if (lone_integer_max(n)) {  // MAX ignores NULLs; over nothing but NULLs it is NULL, as over no rows
                d[(size_t)n->aggs[0].arg] = 1;
            } else if (n->group.empty() && !n->aggs.empty()) {
                // every other list: a row may go only when EVERY aggregate skips it -- all of them take this one column (COUNT(*) counts the
                // row whatever it holds; SUM(a), COUNT(b) would lose b's row with a's NULL).  Otherwise the column travels with validity bytes.
                const int c = n->aggs[0].arg;
                bool all = c >= 0;
                for (auto &a : n->aggs) all = all && a.arg == c && a.arg2 < 0;
                if (all) d[(size_t)c] = 1;
            }
            mark_null_droppable(p, n->in[0].get(), d);
            break;
        }
        case NKind::Join: {
            const size_t nl = n->in[0]->schema.size();
            // Inner: NULL keys never match.  Semi / Anti: `droppable` speaks of the left columns alone.  A NULL key never matches: the right rows it
            // sits in can go, and so can Semi's left rows -- but an ANTI join KEEPS its NULL-keyed left rows (relops.hpp A-S4): their key columns
            // arrive with validity bytes and the probe reads them
            // Cross: the node itself makes nothing droppable (a NULL row of either side is a row of the result, L x R counts it); what an ancestor may
            // drop passes through as through an inner join's non-key columns: a row (i, j) whose column c is NULL is dropped above exactly when every pair
            // of the source row is, and anything below that counts rows (Aggregate, Limit, Window) resets the marks on its own
            const bool inner = n->join_type == JoinType::Inner || n->join_type == JoinType::Cross;
            std::vector<char> l(droppable.begin(), droppable.begin() + nl), r(n->in[1]->schema.size(), 0);
            if (inner) r.assign(droppable.begin() + nl, droppable.end());
            for (auto &k : n->on) {
                if (n->join_type != JoinType::Anti) l[(size_t)k.l] = 1;
                r[(size_t)k.r] = 1;
            }
            mark_null_droppable(p, n->in[0].get(), l);
            mark_null_droppable(p, n->in[1].get(), r);
            break;
        }
        case NKind::Repartition:
        case NKind::Sort:   // (the order of the rows that remain does not depend on the rows that were dropped)
            mark_null_droppable(p, n->in[0].get(), droppable);
            break;
        case NKind::Limit:  // WHICH rows make the first n depends on every row below: nothing may be dropped early
        case NKind::Window: // ... and so does every row's number
            mark_null_droppable(p, n->in[0].get(), std::vector<char>(n->in[0]->schema.size(), 0));
            break;
        case NKind::Union:  // by position: a row dropped below is the row dropped above
            for (auto &c : n->in) mark_null_droppable(p, c.get(), droppable);
            break;
    }
}

inline void mark_co_partitioned(Plan *p, const Node *n, bool under) {
    switch (n->kind) {
        case NKind::Scan:
            if (under) p->leaves[(size_t)n->leaf].co_partitioned = true;
            return;
        case NKind::Repartition:   // this plan places the rows itself from here on
            under = false;
            break;
        case NKind::Join:
            if (n->join_partitioned) under = true;
            break;
        case NKind::Aggregate:
            if (n->mode == AggMode::FinalPartitioned && !n->single_pass) under = true;   // (a single pass groups the rows itself, wherever they were placed)
            break;
        default:
            break;
    }
    for (auto &c : n->in) mark_co_partitioned(p, c.get(), under);
}

// (union.hpp A-U7) leaves with identical field lists are one relation scanned more than once; fed as ONE source, every scan but the first reads the
// fed leaf (Exec::resolve_leaf), which must then hold every column any of them reads: the OR of their `needed` masks.  A row that one of them could
// drop for a NULL is still a row of the others: the AND of their null_droppable marks.
inline void share_leaf_masks(Plan *p) {
    auto same = [](const Leaf &a, const Leaf &b) {
        if (a.schema.size() != b.schema.size()) return false;
        for (size_t c = 0; c < a.schema.size(); ++c)
            if (a.schema[c].name != b.schema[c].name || a.schema[c].type != b.schema[c].type || a.schema[c].is_ts != b.schema[c].is_ts) return false;
        return true;
    };
    for (size_t a = 0; a < p->leaves.size(); ++a)
        for (size_t b = a + 1; b < p->leaves.size(); ++b) {
            Leaf &x = p->leaves[a], &y = p->leaves[b];
            if (!same(x, y) || x.needed.size() != y.needed.size() || x.null_droppable.size() != y.null_droppable.size()) continue;
            for (size_t c = 0; c < x.needed.size(); ++c) {
                x.needed[c] = y.needed[c] = x.needed[c] | y.needed[c];
                x.null_droppable[c] = y.null_droppable[c] = x.null_droppable[c] & y.null_droppable[c];
            }
        }
}

inline bool build_plan(const JValue *root, Plan *plan) {
    Builder b{plan, {}};
    plan->root = b.node(root);
    if (!plan->root) {
        plan->why = b.err.empty() ? "unsupported plan" : b.err;
        return false;
    }
    mark_required(plan, plan->root.get(), std::vector<char>(plan->root->schema.size(), 1));
    mark_null_droppable(plan, plan->root.get(), std::vector<char>(plan->root->schema.size(), 0));
    mark_co_partitioned(plan, plan->root.get(), false);
    if (plan->has_union) share_leaf_masks(plan);
    return true;
}

}  // namespace ir
}  // namespace flockgpu
