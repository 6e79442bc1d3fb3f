"""Random plans inside the claimed dialect, for tests/test_plan_differential.py: case(stratum, seed, i) -> Case(plan, tables, batch_cuts, ordered, note),
a pure function of its three arguments (random.Random and numpy's default_rng seeded from them), so that a failure reproduces without a GPU.

Exactness instead of tolerances.  In every stratum but `float_special`, Float64 inputs are k / 4 with |k| < 2^20 (every sum of up to 2^20 of them is
exact in any order), never NaN and never both zeros in one column; `float_special` alone draws its Float64 columns from float_order_ref.SPECIALS -- NaNs
of four patterns, both zeros, both infinities, subnormals, +-DBL_MAX -- and only orders, compares, casts and MIN / MAXes them (MIN / MAX never see a
NaN: column `a_f2`).  Float64 literals are multiples of 1 / 4 or divisors whose quotient is ONE correctly rounded IEEE division; SUM and AVG
arguments are integers below 2^31 in magnitude, so every sum stays inside 64 bits and inside Float64's 53, and AVG is one correctly rounded division --
except in `group_wide`, whose column `w` (SUM only, Int64 near 2^62) wraps on purpose.  Integer arithmetic wraps as generic_ops.eval_typed says.
Zero divisors, INT_MIN / -1 and casts that do not fit are kept out (divisor literals are never 0 or -1, Float64 values fit Int32) except in `errors`.
The text casts are exact by nature (digits in, digits out); under cast_expr every timestamp lies in the years 0000 to 9999 and every text parses
(text_numbers(valid=True) keeps only what parse_text_ref.parse_one takes); what does not stands under try_cast_expr alone -- except in `errors_text`;
SUM / MIN / MAX over parsed values take texts of magnitude below 2^31 (`parse_text` case 4), the rule of the other sums.

Order.  `ordered` is True only when the root is a sort or a limit over a sort, or a union over scans, filters and projections (ordered_union: the
rows of input 0 in their order, then input 1's; a filter keeps its input's order).  Such a sort carries the row-unique column `id` (or a GROUP BY's
key tuple, or every column of its input) as its last key.  Everything else is compared as a multiset; no limit sits over an unsorted input.

Shapes.  Row counts come from SIZES (the flag tile and kDenseTile 8192, the sort tile 4096) plus one case of 20 011 and one of 32 769 rows per stratum
(case 4 of seed 0 / seed 1); join build sides from both sides of kTinyBuild = 4096.  Every stratum is DIRECTED by the case number i: case i takes the
i-th way through the node it is about (the docstring of each recipe says which), the random part draws everything else.

Columns of a table with prefix `p`: p_k Int32 and p_l Int64 (keys in the case's style), p_g Int32 (a small dense key), p_u UInt64 (either side of 2^63),
p_t Timestamp(ms) (either side of 1970), p_f Float64, p_s / p_s2 Utf8, p_v Int64 and p_i Int32 (values below 2^20 / of any size), p_id Int64 (the row's
number, never NULL).  Every other column is NULL with a share drawn from NULL_SHARES.  The strata of the text casts put directed values into these
columns (number_pools) and add the Utf8 columns of PARSE_COLS (parse_table)."""
import collections
import random

import numpy as np

import float_order_ref as fo

Case = collections.namedtuple("Case", "plan tables batch_cuts ordered note")

TS = {"Timestamp": ["Millisecond", None]}
SIZES = [0, 1, 63, 64, 65, 700, 4095, 4096, 4097, 8191, 8192, 8193]
BUILD_SIZES = [1, 300, 4096, 4097, 9000]
NULL_SHARES = [0.0, 0.02, 0.3, 1.0]
KEY_STYLES = ["dense", "dense_offset", "sparse", "constant", "unique", "hot"]
WORDS = ["", "7", "07", "a", "ab", "abc", "prefix_8", "prefix_8x", "sixteen_bytes_pfx", "sixteen_bytes_pfxa", "sixteen_bytes_pfxb", "x" * 17, "y" * 17 + "z",
         "z" * 40, "w" * 70, "w" * 69 + "v", "été", "€", "\U0001F600", "aé€\U0001F600", "a/b/c", " pad ", "a//b", "xx/é/yy"]
CASES_PER_SEED = 6
STRATA = ["filter_project", "text", "group_narrow", "group_composite", "group_wide", "distinct_count", "global_agg", "join_inner", "join_semi_anti",
          "sort_limit", "window", "cross", "mixed", "errors", "union", "cast_text", "parse_text", "errors_text",
          "float_special"]                   # (appended: _rngs seeds from STRATA.index, so every earlier stratum's cases stay what they were)

# The kernels every (stratum, seed) must run, by name as profile_read() gives them; `sort_emit_kernel` is a template with an instance per digit
# width whose profile name may carry the width: names are matched by PREFIX.
MUST_RUN = {
    "filter_project": ("pred_flag_kernel", "valprog_kernel", "strmatch_rows_kernel", "strmatch_contains_kernel", "utf8_chars_kernel"),
    "text": ("textsel_len_kernel", "textsel_emit_kernel", "text_slice_stream_kernel", "text_slice_general_kernel"),
    "group_narrow": ("dense_group_kernel", "group_insert_n_kernel", "pack_pair_kernel"),
    "group_composite": ("key_codes_insert_kernel", "utf8_codes_build_kernel"),
    "group_wide": ("wide_group_kernel", "wide_group_finish_kernel"),
    "distinct_count": ("distinct_insert_kernel",),
    "global_agg": ("global_reduce_kernel", "global_fold_kernel"),
    "join_inner": ("join_tiny_kernel", "join_build_dense_kernel", "join_probe_unique_flag_kernel", "join_probe_dense_kernel", "join_hash_build_kernel",
                   "join_hash_probe_flag_kernel", "join_hash_probe_kernel", "key_codes_probe_kernel"),
    "join_semi_anti": ("semi_tiny_kernel", "semi_bitmap_build_kernel", "semi_probe_bitmap_flag_kernel", "semi_set_build_kernel", "semi_probe_set_flag_kernel",
                       "semi_ids_flag_kernel"),
    # (compose_perm_kernel is launched outside a LaunchScope -- relops.hip sort_rows, `pass` --, so no profile names it; it follows every
    # sort_norm_kernel pass whose sub-key takes more than one value)
    "sort_limit": ("sort_emit_kernel", "sort_int_digit_kernel", "sort_norm_kernel"),
    "window": ("win_tile_kernel", "win_carry_kernel", "win_emit_kernel", "run_rank_kernel"),
    "cross": ("cross_repeat_kernel", "cross_tile_kernel"),
    "mixed": (),
    "errors": (),
    "union": ("union_fixed_kernel", "union_valid_kernel", "union_bytes_kernel", "union_offsets_kernel"),
    "cast_text": ("numtext_len_kernel", "numtext_emit_kernel"),
    "parse_text": ("textnum_parse_kernel",),
    "errors_text": (),
    "float_special": ("sort_norm_kernel", "win_tile_kernel", "win_carry_kernel", "win_emit_kernel", "run_rank_kernel", "pred_flag_kernel", "valprog_kernel"),
}


# ------------------------------------------------------------------ plan JSON
def dt(t):
    return TS if t == "ts" else t


def field(name, t):
    return {"data_type": dt(t), "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": True}


def schema(cols):
    return {"fields": [field(n, t) for n, t in cols], "metadata": {}}


def col(name, cols):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def lit(kind, v):
    return {"physical_expr": "literal", "value": {kind: v}}


def binop(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def cast(e, t, safe=False):
    return {"physical_expr": "try_cast_expr" if safe else "cast_expr", "expr": e, "cast_type": dt(t)}


def fn(name, ret, *args):
    return {"physical_expr": "scalar_function_expr", "name": name, "args": list(args), "return_type": dt(ret)}


def case_(whens, els=None, base=None):
    return {"physical_expr": "case_expr", "expr": base, "when_then_expr": [[w, t] for w, t in whens], "else_expr": els}


def coalesce(inp):
    return {"execution_plan": "coalesce_batches_exec", "input": inp, "target_batch_size": 4096}


class Node:
    """a plan and the columns [(name, type)] it gives"""
    def __init__(self, plan, cols):
        self.plan, self.cols = plan, list(cols)

    def c(self, name):
        return col(name, self.cols)

    def ty(self, name):
        return dict(self.cols)[name]


def scan(cols, projection=None):
    p = {"execution_plan": "memory_exec", "schema": schema(cols), "projection": list(range(len(cols))) if projection is None else projection}
    return Node(p, cols if projection is None else [cols[k] for k in projection])


def filt(inp, pred):
    return Node(coalesce({"execution_plan": "filter_exec", "predicate": pred, "input": inp.plan}), inp.cols)


def proj(inp, exprs):
    """exprs: [(expression, name, type)]"""
    out = [(n, t) for _, n, t in exprs]
    return Node({"execution_plan": "projection_exec", "expr": [[e, n] for e, n, _ in exprs], "input": inp.plan, "schema": schema(out)}, out)


def keep(inp, names):
    return proj(inp, [(inp.c(n), n, inp.ty(n)) for n in names])


def sort(inp, keys):
    """keys: [(column name, descending, nulls_first)]"""
    return Node({"execution_plan": "sort_exec", "input": inp.plan,
                 "expr": [{"expr": inp.c(k), "options": {"descending": d, "nulls_first": nf}} for k, d, nf in keys]}, inp.cols)


def limit(inp, n):
    return Node({"execution_plan": "global_limit_exec", "limit": n, "input": inp.plan}, inp.cols)


def hashed(inp, key):
    return coalesce({"execution_plan": "repartition_exec", "input": inp.plan, "partitioning": {"Hash": [[inp.c(key)], 4]}})


def join(jt, left, right, on):
    out = left.cols + (right.cols if jt == "Inner" else [])
    return Node({"execution_plan": "hash_join_exec", "left": hashed(left, on[0][0]), "right": hashed(right, on[0][1]), "join_type": jt, "mode": "Partitioned",
                 "on": [[left.c(a), right.c(b)] for a, b in on], "schema": schema(out)}, out)


def cross(left, right):
    out = left.cols + right.cols
    return Node({"execution_plan": "cross_join_exec", "left": left.plan, "right": right.plan, "schema": schema(out)}, out)


def result_type(f, t):
    return "UInt64" if f in ("count", "dc") else "Float64" if f == "avg" else ("UInt64" if t == "UInt64" else "Int64") if f == "sum" else t


def aggregate(inp, keys, aggs, key_exprs=None, single=None):
    """Partial -> Hash repartition -> FinalPartitioned (no keys: Partial -> CoalescePartitions -> Final), as the planner writes it.
    aggs: [(fn, column name or None for COUNT(*) or (expression, type))], fn 'dc' = COUNT(DISTINCT); key_exprs: {key name: (expression, type)}.
    single: 'Partial' gives that node alone."""
    key_exprs = key_exprs or {}
    entries, out, states = [], [], []
    for k, (f, arg) in enumerate(aggs):
        if arg is None:
            e, at, label = lit("UInt8", 1), None, "UInt8(1)"
        elif isinstance(arg, tuple):
            e, at, label = arg[0], arg[1], "expr"
        else:
            e, at, label = inp.c(arg), inp.ty(arg), arg
        name = "a%d:%s(%s)" % (k, "COUNT DISTINCT" if f == "dc" else f.upper(), label)
        rt = result_type(f, at)
        if f == "dc":
            entries.append({"aggregate_expr": "distinct_count", "name": name, "data_type": "UInt64", "nullable": True, "exprs": [e],
                            "state_data_types": [dt(at)], "input_data_types": [dt(at)]})
            item = {"data_type": dt(at), "dict_id": 0, "dict_is_ordered": False, "name": "item", "nullable": True}
            states.append({"data_type": {"List": item}, "dict_id": 0, "dict_is_ordered": False, "name": name + "[count distinct]", "nullable": False})
        else:
            entries.append({"aggregate_expr": f, "name": name, "data_type": dt(rt), "nullable": True, "expr": e})
            states += [field(name + "[count]", "UInt64"), field(name + "[sum]", "Float64")] if f == "avg" else [field("%s[%s]" % (name, f), rt)]
        out.append((name, rt))
    kcols = [(k, key_exprs[k][1] if k in key_exprs else inp.ty(k)) for k in keys]
    group = [[key_exprs[k][0] if k in key_exprs else inp.c(k), k] for k in keys]
    kf = [field(k, t) for k, t in kcols]
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": group, "aggr_expr": entries, "input": inp.plan,
            "input_schema": schema(inp.cols), "schema": {"fields": kf + states, "metadata": {}}}
    if single == "Partial":
        pcols = list(kcols)
        for (f, arg), (name, rt) in zip(aggs, out):
            pcols += [(name + "[count]", "UInt64"), (name + "[sum]", "Float64")] if f == "avg" else [("%s[%s]" % (name, f), rt)]
        return Node(part, pcols)
    if keys:
        mid = coalesce({"execution_plan": "repartition_exec", "input": part,
                        "partitioning": {"Hash": [[{"physical_expr": "column", "name": k, "index": j} for j, k in enumerate(keys)], 4]}})
    else:
        mid = {"execution_plan": "coalesce_partitions_exec", "input": part}
    final = {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned" if keys else "Final",
             "group_expr": [[{"physical_expr": "column", "name": k, "index": j}, k] for j, k in enumerate(keys)], "aggr_expr": entries, "input": mid,
             "input_schema": schema(inp.cols), "schema": schema(kcols + out)}
    return Node(final, kcols + out)


def window(inp, entries):
    """entries: [(fn or 'row_number', argument column or None, partition columns, order columns)]; the window columns come first"""
    ws, out = [], []
    for k, (f, arg, part, order) in enumerate(entries):
        pb = [inp.c(p) for p in part]
        ob = [{"expr": inp.c(o), "options": {"descending": False, "nulls_first": False}} for o in order]
        if f == "row_number":
            name = "w%d:rn" % k
            ws.append({"window_expr": "built_in_window_expr", "fun": "RowNumber", "name": name, "partition_by": pb, "order_by": ob})
            out.append((name, "UInt64"))
            continue
        at = inp.ty(arg) if arg else None
        name = "w%d:%s(%s)" % (k, f.upper(), arg or "UInt8(1)")
        rt = result_type(f, at)
        ws.append({"window_expr": "aggregate_window_expr", "partition_by": pb, "order_by": ob,
                   "aggregate": {"aggregate_expr": f, "name": name, "data_type": dt(rt), "nullable": True, "expr": inp.c(arg) if arg else lit("UInt8", 1)}})
        out.append((name, rt))
    return Node({"execution_plan": "window_agg_exec", "input": inp.plan, "window_expr": ws}, out + inp.cols)


# ------------------------------------------------------------------ tables
_RANGE = {"Int32": (-2**31, 2**31 - 1), "Int64": (-2**63, 2**63 - 1), "UInt64": (0, 2**64 - 1)}


def key_values(style, n, ty, r, card):
    """n key values of integer type `ty` in one of KEY_STYLES over about `card` distinct values"""
    lo, hi = _RANGE[ty]
    card = max(1, card)
    if style == "unique":
        return [int(x) * 3 - 7 for x in r.permutation(n)] if ty != "UInt64" else [int(x) * 3 for x in r.permutation(n)]
    if style == "constant":
        return [42] * n
    d = [int(x) for x in r.integers(0, card, n)]
    if style == "dense":
        return [x + (0 if ty == "UInt64" else -card // 3) for x in d]
    if style == "dense_offset":
        return [hi - x for x in d] if r.random() < 0.5 else [lo + x for x in d]
    if style == "hot":
        hot = r.random(n) < 0.5
        return [5 if h else x for x, h in zip(d, hot)]
    assert style == "sparse", style
    pool = [int(x) for x in r.integers(lo // 2, hi // 2, card, dtype=np.int64)] if ty != "UInt64" else [int(x) for x in r.integers(0, 2**63 - 1, card)]
    if ty == "UInt64":
        pool = [x * 2 + 1 for x in pool]
    return [pool[x] for x in d]


def with_nulls(vals, share, r):
    if share <= 0:
        return list(vals)
    if share >= 1:
        return [None] * len(vals)
    m = r.random(len(vals)) < share
    return [None if m[k] else v for k, v in enumerate(vals)]


def word(x):
    x = int(x)
    return WORDS[x % len(WORDS)] + ("" if x < len(WORDS) else "%d" % (x // len(WORDS)))


COLS = [("k", "Int32"), ("l", "Int64"), ("g", "Int32"), ("u", "UInt64"), ("t", "ts"), ("f", "Float64"), ("s", "Utf8"), ("s2", "Utf8"), ("v", "Int64"), ("i", "Int32"),
        ("id", "Int64")]


def table_cols(prefix):
    return [(prefix + "_" + n, t) for n, t in COLS]


def make_table(prefix, n, r, rnd, style=None, card=None, nulls=None, groups=None, key_nulls=None):
    """-> {column: [values]} with the columns of table_cols(prefix).  style / card: of the key columns k and l; groups: distinct values of g;
    nulls: {column: share} overriding the drawn shares; key_nulls: the share of k, l, g, s (drawn like the others when None)."""
    style = style or rnd.choice(KEY_STYLES)
    card = card if card is not None else rnd.choice([1, 7, 300, 2047, 2049, max(1, n)])
    groups = groups or rnd.choice([1, 5, 37])
    base = key_values(style, n, "Int32", r, card)
    t = {"k": base,
         "l": key_values(style, n, "Int64", r, card),
         "g": [int(x) for x in r.integers(0, groups, n)],
         "u": [2**63 - 5 + int(x) for x in r.integers(0, 11, n)],
         "t": [int(x) for x in r.integers(-400 * 86_400_000, 20_000 * 86_400_000, n)],
         "f": [int(x) / 4 for x in r.integers(-2**20 + 1, 2**20, n)],
         "s": [word(x) for x in r.integers(0, max(1, min(card, 4 * len(WORDS))), n)],
         "s2": [WORDS[int(x)] for x in r.integers(0, len(WORDS), n)],
         "v": [int(x) for x in r.integers(-2**20 + 1, 2**20, n)],
         "i": [int(x) for x in r.integers(-2**31, 2**31, n)],
         "id": list(range(n))}
    zero = [k for k, x in enumerate(t["f"]) if x == 0]
    for k in zero:
        t["f"][k] = 0.25                                        # (no zero at all: never both zeros, and a column may be a Float64 divisor nowhere)
    out = {}
    for name, _ in COLS:
        share = rnd.choice(NULL_SHARES[:3] + NULL_SHARES[:3] + [1.0]) if name != "id" else 0.0
        if key_nulls is not None and name in ("k", "l", "g", "s"):
            share = key_nulls
        if nulls and name in nulls:
            share = nulls[name]
        out[prefix + "_" + name] = with_nulls(t[name], share, r)
    return out


def cuts(n, r, rnd):
    """batch boundaries 0 = c0 <= c1 <= ... = n: a few random cuts, an empty batch, a cut one row off a tile boundary"""
    c = sorted(int(x) for x in r.integers(0, n + 1, rnd.choice([1, 2, 4])))
    if c:
        c.append(c[rnd.randrange(len(c))])                      # the same cut twice: an empty batch
    for tile in (4096, 8192):
        if n > tile + 1:
            c.append(tile + rnd.choice([-1, 1]))
    return [0] + sorted(c) + [n]


def size(seed, i, rnd, choices=SIZES):
    if i == 4 and seed % 4 == 0:
        return 20_011
    if i == 4 and seed % 4 == 1:
        return 32_769
    return rnd.choice(choices)


# ------------------------------------------------------------------ expressions
DIVISORS = [2, 3, 7, -3, -7, 1000]
LIKES = ["a%", "%b%", "%w%", "_", "é_%", "%_é%", "prefix_8%", "%z", "_7", "%/%/%", "", "%"]


class Exprs:
    """random expressions over the columns of one table prefix, inside the claimed dialect; no operator stands over literals alone"""
    def __init__(self, node, prefix, rnd):
        self.n, self.p, self.r = node, prefix, rnd

    def nl(self, e, name):
        return self.c(name) if e["physical_expr"] == "literal" else e

    def c(self, name):
        return self.n.c(self.p + "_" + name)

    def int32(self, d):
        r = self.r
        if d <= 0 or r.random() < 0.25:
            return r.choice([self.c("k"), self.c("i"), self.c("g"), lit("Int32", r.choice([0, 1, -5, 70_000, 2**31 - 1]))])
        pick = r.random()
        if pick < 0.45:
            return binop(self.nl(self.int32(d - 1), "i"), r.choice(["Plus", "Minus", "Multiply"]), self.int32(d - 1))
        if pick < 0.6:
            return binop(self.nl(self.int32(d - 1), "k"), r.choice(["Divide", "Modulo"]), lit("Int32", r.choice(DIVISORS)))
        if pick < 0.7:
            return {"physical_expr": "negative_expr", "arg": self.nl(self.int32(d - 1), "g")}
        if pick < 0.8:
            return r.choice([fn("char_length", "Int32", self.c("s")), fn("octet_length", "Int32", self.c("s2")),
                             fn("date_part", "Int32", lit("Utf8", r.choice(["year", "month", "day", "hour", "minute", "second", "dow", "doy"])), self.c("t"))])
        if pick < 0.9:
            return case_([(self.boolean(d - 1), self.int32(d - 1))], self.int32(d - 1) if r.random() < 0.7 else None)
        return cast(self.c("f"), "Int32", safe=r.random() < 0.5)

    def int64(self, d):
        r = self.r
        if d <= 0 or r.random() < 0.25:
            return r.choice([self.c("v"), self.c("l"), self.c("id"), lit("Int64", r.choice([0, 3, -2**40, 2**62]))])
        pick = r.random()
        if pick < 0.45:
            return binop(self.nl(self.int64(d - 1), "v"), r.choice(["Plus", "Minus", "Multiply"]), self.int64(d - 1))
        if pick < 0.6:
            return binop(self.nl(self.int64(d - 1), "l"), r.choice(["Divide", "Modulo"]), lit("Int64", r.choice(DIVISORS)))
        if pick < 0.8:
            return cast(self.nl(self.int32(d - 1), "k"), "Int64")
        return case_([(self.boolean(d - 1), self.int64(d - 1))], self.int64(d - 1) if r.random() < 0.7 else None)

    def float64(self, d):
        r = self.r
        if d <= 0 or r.random() < 0.25:
            return r.choice([self.c("f"), lit("Float64", r.choice([0.25, -1.5, 3.0, 1024.0]))])
        pick = r.random()
        if pick < 0.3:
            return binop(self.nl(self.float64(d - 1), "f"), r.choice(["Plus", "Minus"]), self.float64(d - 1))
        if pick < 0.4:
            return binop(self.nl(self.float64(d - 1), "f"), "Multiply", lit("Float64", r.choice([0.5, -2.0, 4.0])))
        if pick < 0.5:
            return binop(self.nl(self.float64(d - 1), "f"), "Divide", lit("Float64", r.choice([3.0, -7.0, 0.5])))
        if pick < 0.8:
            name = r.choice(["abs", "signum", "floor", "ceil", "round", "trunc", "sqrt"])
            arg = self.nl(self.float64(d - 1), "f")
            return fn(name, "Float64", fn("abs", "Float64", arg) if name == "sqrt" else arg)      # (no NaN: sqrt of a magnitude)
        return cast(self.nl(self.int32(d - 1), "i"), "Float64")

    def ts(self, d):
        r = self.r
        if d <= 0 or r.random() < 0.4:
            return self.c("t")
        return fn("date_trunc", "ts", lit("Utf8", r.choice(["second", "minute", "hour", "day", "week", "month", "year"])), self.c("t"))

    def simple(self, d):
        """a predicate of the leaves the one-pass predicate program takes -- a column (or its remainder) against a literal, IN, IS [NOT] NULL of a
        column, LIKE, a Utf8 column against a literal -- under AND / OR / NOT.  LIKE and the Utf8 comparisons stand beside such leaves only: a
        predicate with a computed leaf runs on the general evaluator, which takes no text (plan.hip compile_filter)"""
        r = self.r
        pick = r.random()
        if d > 0 and pick < 0.35:
            return binop(self.simple(d - 1), r.choice(["And", "Or"]), self.simple(d - 1))
        if d > 0 and pick < 0.42:
            return {"physical_expr": "not_expr", "arg": self.simple(d - 1)}
        cmp = lambda: r.choice(["Eq", "NotEq", "Lt", "LtEq", "Gt", "GtEq"])
        return r.choice([
            lambda: binop(self.c(r.choice(["k", "g", "i"])), cmp(), lit("Int32", r.choice([0, 3, -5, 40]))),
            lambda: binop(self.c(r.choice(["v", "l", "id"])), cmp(), lit("Int64", r.choice([0, 100, -2**40]))),
            lambda: binop(self.c("f"), cmp(), lit("Float64", r.choice([0.25, -1000.5, 3.0]))),
            lambda: binop(binop(self.c(r.choice(["k", "i"])), "Modulo", lit("Int32", r.choice([2, 3, 7]))), "Eq", lit("Int32", r.choice([0, 1, -1]))),
            lambda: {"physical_expr": "in_list_expr", "expr": self.c(r.choice(["g", "k"])), "list": [lit("Int32", x) for x in r.sample(range(-3, 12), 3)],
                     "negated": r.random() < 0.3},
            lambda: {"physical_expr": r.choice(["is_null_expr", "is_not_null_expr"]), "arg": self.c(r.choice(["s", "f", "i", "t"]))},
            lambda: binop(self.c(r.choice(["s", "s2"])), r.choice(["Like", "NotLike"]), lit("Utf8", r.choice(LIKES))),
            lambda: binop(self.c(r.choice(["s", "s2"])), r.choice(["Lt", "LtEq", "Gt", "GtEq"]), lit("Utf8", r.choice(WORDS))),
            lambda: binop(lit("Utf8", r.choice(WORDS)), r.choice(["Lt", "GtEq"]), self.c(r.choice(["s", "s2"])))])()

    def boolean(self, d):
        """a predicate over computed values (no text in it: see `simple`)"""
        r = self.r
        pick = r.random()
        if d <= 0 or pick < 0.35:
            kind = r.choice(["Int32", "Int64", "Float64"])
            a = self.nl({"Int32": self.int32, "Int64": self.int64, "Float64": self.float64}[kind](d - 1), {"Int32": "k", "Int64": "v", "Float64": "f"}[kind])
            b = {"Int32": self.int32, "Int64": self.int64, "Float64": self.float64}[kind](0)
            return binop(a, r.choice(["Eq", "NotEq", "Lt", "LtEq", "Gt", "GtEq"]), b)
        if pick < 0.5:
            return binop(self.boolean(d - 1), r.choice(["And", "Or"]), self.boolean(d - 1))
        if pick < 0.57:
            return {"physical_expr": "not_expr", "arg": self.boolean(d - 1)}
        if pick < 0.67:
            return {"physical_expr": r.choice(["is_null_expr", "is_not_null_expr"]), "arg": r.choice([self.c("v"), self.c("f"), self.nl(self.int32(d - 1), "i")])}
        if pick < 0.77:
            return {"physical_expr": "in_list_expr", "expr": self.c(r.choice(["g", "k"])), "list": [lit("Int32", x) for x in r.sample(range(-3, 12), 3)],
                    "negated": r.random() < 0.3}
        return binop(self.ts(1), r.choice(["Lt", "GtEq", "Eq"]), self.ts(1))       # a Timestamp against a truncated one

    def text(self, d):
        """a text-valued expression: a literal, a column, a slice of a column, a CASE of such"""
        r = self.r
        pick = r.random()
        if d <= 0 or pick < 0.2:
            return r.choice([self.c("s"), self.c("s2"), lit("Utf8", r.choice(WORDS))])
        if pick < 0.6:
            return self.slice(r.randint(1, 2))
        whens = [(self.plain_boolean(), self.text(d - 1) if k == 0 or r.random() < 0.7 else {"physical_expr": "literal", "value": None}) for k in range(r.randint(1, 3))]
        return case_(whens, self.text(d - 1) if r.random() < 0.6 else None)

    def plain_boolean(self):
        """a condition without text in it (text inside a condition of a text CASE stays refused)"""
        r = self.r
        a = binop(r.choice([self.c("g"), self.c("k"), self.c("i")]), r.choice(["Lt", "GtEq", "Eq"]), lit("Int32", r.choice([0, 2, 5])))
        if r.random() < 0.4:
            a = binop(a, r.choice(["And", "Or"]), binop(self.c("f"), "Gt", lit("Float64", 0.0)))
        return a

    def slice(self, d):
        r = self.r
        arg = self.c(r.choice(["s", "s2"])) if d <= 1 else self.slice(d - 1)
        name = r.choice(["split_part", "split_part", "left", "right", "ltrim", "rtrim", "btrim"])
        if name == "split_part":
            return fn(name, "Utf8", arg, lit("Utf8", r.choice(["/", "//", "é", "_"])), lit("Int64", r.randint(1, 3)))
        if name in ("left", "right"):
            return fn(name, "Utf8", arg, lit("Int64", r.choice([-2, 0, 1, 3, 17])))
        if r.random() < 0.5:
            return fn(name, "Utf8", arg)
        return fn(name, "Utf8", arg, lit("Utf8", r.choice(["x", " a", "wé", "€"])))


# ------------------------------------------------------------------ strata
def _rngs(stratum, seed, i):
    h = (STRATA.index(stratum) * 1000 + seed) * 100 + i
    return random.Random(h), np.random.default_rng(h)


def _one_table(prefix, n, r, rnd, **kw):
    t = make_table(prefix, n, r, rnd, **kw)
    return scan(table_cols(prefix)), t


def _finish(node, tables, r, rnd, ordered, note):
    sizes = [len(next(iter(t.values()))) for t in tables]
    return Case(node.plan, tables, [cuts(n, r, rnd) for n in sizes], ordered, note)


def r_filter_project(seed, i, rnd, r):
    """case 0: a LIKE '%needle%' beside other leaves of the predicate program; case 1: other LIKE forms and a Utf8 comparison; case 2: text lengths; others: random
    predicates and projected expressions of depth up to 4"""
    n = size(seed, i, rnd, SIZES[1:] if i < 3 else SIZES)
    nulls = {"s": rnd.choice([0.0, 0.02, 0.3]), "s2": rnd.choice([0.0, 0.3]), "t": 0.02, "f": 0.02, "i": 0.02, "k": 0.02} if i < 4 else None
    a, t = _one_table("a", n, r, rnd, nulls=nulls)
    x = Exprs(a, "a", rnd)
    depth = 2 if n > 10_000 else rnd.randint(2, 4)
    if i == 0:
        pred = binop(binop(x.c("s2"), "Like", lit("Utf8", rnd.choice(["%w%", "%b%", "%é%"]))), rnd.choice(["And", "Or"]), x.simple(depth - 1))
    elif i == 1:
        pred = binop(binop(x.c("s2"), rnd.choice(["Like", "NotLike"]), lit("Utf8", rnd.choice(["_", "a_€%", "_7", "é_%"]))), "Or",
                     binop(x.c("s"), rnd.choice(["Lt", "GtEq"]), lit("Utf8", rnd.choice(WORDS))))
    elif i == 2:
        pred = binop(binop(fn("char_length", "Int32", x.c("s")), "Lt", fn("octet_length", "Int32", x.c("s"))), "Or", x.boolean(depth - 1))
    else:
        pred = x.simple(depth) if rnd.random() < 0.5 else x.boolean(depth)
    out = [(x.c("id"), "id", "Int64")]
    makers = [("Int32", x.int32), ("Int64", x.int64), ("Float64", x.float64), ("ts", x.ts)]
    if i == 3:      # the rules the arithmetic quirks are about, on values where they differ
        out += [(binop(x.c("v"), "Divide", lit("Int64", 7)), "q", "Int64"), (binop(x.c("v"), "Modulo", lit("Int64", -7)), "m", "Int64"),
                (binop(x.c("i"), "Multiply", lit("Int32", 3)), "w", "Int32"),
                (fn("date_trunc", "ts", lit("Utf8", "week"), x.c("t")), "wk", "ts"), (fn("date_trunc", "ts", lit("Utf8", "hour"), x.c("t")), "hr", "ts")]
    for k in range(rnd.randint(1, 4)):
        ty, make = rnd.choice(makers)
        out.append((make(depth), "e%d" % k, ty))
    node = proj(filt(a, pred), out) if rnd.random() < 0.8 or i < 4 else filt(proj(a, out + [(x.c("s"), "a_s", "Utf8")]), binop(col("id", [("id", "Int64")]), "GtEq", lit("Int64", 0)))
    return _finish(node, [t], r, rnd, False, "n=%d depth=%d" % (n, depth))


def r_text(seed, i, rnd, r):
    """case 0: a CASE of literals and columns; case 1: one-byte delimiters and trims (the streaming slice kernel); case 2: a two-byte delimiter and a
    non-ASCII trim set (the general slice kernel); case 3: left / right over multi-byte text and a CASE whose condition is NULL for some rows;
    others: random text expressions as projected columns and as a GROUP BY key"""
    n = size(seed, i, rnd, SIZES[1:] if i < 4 else SIZES)
    a, t = _one_table("a", n, r, rnd, nulls={"s": rnd.choice([0.0, 0.3]), "s2": 0.02, "g": 0.3 if i == 3 else 0.02, "k": 0.02, "i": 0.02, "f": 0.02})
    x = Exprs(a, "a", rnd)
    if i == 0:
        es = [case_([(x.plain_boolean(), lit("Utf8", "low")), (x.plain_boolean(), x.c("s"))], rnd.choice([None, x.c("s2"), lit("Utf8", "")]))]
    elif i == 1:
        es = [fn("split_part", "Utf8", x.c("s2"), lit("Utf8", "/"), lit("Int64", 2)), fn("btrim", "Utf8", x.c("s2")), fn("rtrim", "Utf8", x.c("s"), lit("Utf8", "xz"))]
    elif i == 2:
        es = [fn("split_part", "Utf8", x.c("s2"), lit("Utf8", "//"), lit("Int64", 2)), fn("ltrim", "Utf8", x.c("s2"), lit("Utf8", "é€"))]
    elif i == 3:
        es = [fn("left", "Utf8", x.c("s2"), lit("Int64", 2)), fn("right", "Utf8", x.c("s2"), lit("Int64", 1)), fn("left", "Utf8", x.c("s"), lit("Int64", -1)),
              case_([(binop(x.c("g"), "GtEq", lit("Int32", 0)), lit("Utf8", "seen"))], x.c("s2"))]
    else:
        es = [x.text(rnd.randint(1, 3)) for _ in range(rnd.randint(1, 3))]
    out = [(x.c("id"), "id", "Int64")] + [(e, "x%d" % k, "Utf8") for k, e in enumerate(es)]
    node = proj(a, out)
    how = rnd.choice(["project", "project", "group", "filter"]) if i >= 1 else "project"
    if how == "group":
        node = aggregate(proj(a, out + [(x.c("v"), "v", "Int64")]), ["x0"], [("count", None), ("sum", "v")])
    elif how == "filter":
        node = proj(filt(a, x.plain_boolean()), out)
    return _finish(node, [t], r, rnd, False, "n=%d %s" % (n, how))


def _narrow_aggs(rnd, n_aggs, p="a"):
    menu = [("count", None), ("count", p + "_f"), ("sum", p + "_v"), ("sum", p + "_i"), ("min", p + "_f"), ("max", p + "_u"), ("min", p + "_t"), ("avg", p + "_v"),
            ("avg", p + "_i"), ("max", p + "_l"), ("min", p + "_i"), ("count", p + "_s")]
    aggs, acc = [], 0
    for f in [rnd.choice(menu) for _ in range(n_aggs)]:          # at most four accumulators, AVG taking two
        if acc + (2 if f[0] == "avg" else 1) <= 4:
            aggs.append(f)
            acc += 2 if f[0] == "avg" else 1
    return aggs


def r_group_narrow(seed, i, rnd, r):
    """1 to 4 accumulators (AVG takes two; `_narrow_aggs` stops at four).  case 0: one Int32 key over a dense range and arguments without NULLs (dense_group_kernel); case 1: one
    sparse Int64 key (group_insert_n_kernel); case 2: an (Int32, Int32) pair without NULLs under at most four accumulators (pack_pair_kernel: plan.hip
    choose_key_shape takes any other two-column key, and any node that needs group ids, to key_codes); case 3: COUNT(col) and AVG over NULLs, over a
    filter and under one (HAVING COUNT(*) > 1); others: every key style, group counts either side of kDenseBins, over a filter, under a HAVING filter and
    under a sort at random"""
    n = size(seed, i, rnd, [65, 700, 4097, 8192, 8193] if i < 4 else SIZES)
    style = {0: "dense", 1: "sparse", 2: "dense"}.get(i, rnd.choice(KEY_STYLES))
    card = rnd.choice([7, 300, 2047, 2049, 5000])
    nulls = {"v": 0.0, "i": 0.0, "f": 0.0, "u": 0.0, "t": 0.0, "l": 0.0, "s": 0.0} if i == 0 else {"v": 0.3, "i": 0.3, "f": 0.3} if i == 3 else None
    a, t = _one_table("a", n, r, rnd, style=style, card=card, nulls=nulls, key_nulls=0.0 if i in (0, 2) else rnd.choice([0.0, 0.02, 0.3]))
    keys = {0: ["a_k"], 1: ["a_l"], 2: ["a_k", "a_g"]}.get(i, [rnd.choice(["a_k", "a_l", "a_g", "a_u", "a_t"])])
    if i == 0:
        aggs = [("count", None), ("sum", "a_v"), ("max", "a_v")]
    elif i == 2:
        aggs = [("count", None), ("sum", "a_i"), ("min", "a_f")]
    elif i == 3:
        aggs = [("count", "a_v"), ("avg", "a_v"), ("count", None)]
    else:
        aggs = _narrow_aggs(rnd, rnd.randint(1, 3))
    inp = a
    if i == 3 or rnd.random() < 0.3:
        inp = filt(a, binop(a.c("a_g"), "GtEq", lit("Int32", rnd.choice([0, 1]))))
    having = i == 3 or (i > 3 and rnd.random() < 0.4)
    if having and ("count", None) not in aggs:
        aggs = [("count", None)] + aggs[:2]
    node = aggregate(inp, keys, aggs)
    if having:                                                   # a filter over the aggregate's output
        node = filt(node, binop(node.c(node.cols[len(keys) + aggs.index(("count", None))][0]), "Gt", lit("UInt64", 1)))
    ordered = i > 3 and rnd.random() < 0.5
    if ordered:
        node = sort(node, [(k, rnd.random() < 0.5, rnd.random() < 0.5) for k in keys])
    return _finish(node, [t], r, rnd, ordered, "n=%d style=%s card=%d keys=%s" % (n, style, card, keys))


def r_group_composite(seed, i, rnd, r):
    """case 0: three keys of mixed types with NULLs (key_codes_insert_kernel); case 1: one Utf8 key (utf8_codes_build_kernel); case 2: a computed key
    beside a column; others: 2 to 8 key columns of mixed types"""
    n = size(seed, i, rnd, [65, 700, 4097, 8193] if i < 3 else SIZES)
    a, t = _one_table("a", n, r, rnd, card=rnd.choice([7, 300, 2049]), key_nulls=0.3 if i == 0 else rnd.choice([0.0, 0.02, 0.3]), nulls={"u": 0.3, "t": 0.02})
    menu = ["a_k", "a_l", "a_g", "a_u", "a_t", "a_s", "a_s2", "a_i"]
    key_exprs = None
    if i == 0:
        keys = ["a_k", "a_s", "a_u"]
    elif i == 1:
        keys = ["a_s"]
    elif i == 2:
        keys = ["a_g", "day"]
        key_exprs = {"day": (fn("date_trunc", "ts", lit("Utf8", "year"), a.c("a_t")), "ts")}
    else:
        keys = rnd.sample(menu, rnd.randint(2, 8))
    # (one Utf8 key runs on utf8_codes only under at most four accumulators: five or more number the groups with key_codes, plan.hip choose_key_shape)
    aggs = [("count", None), ("min", "a_f")] if i == 1 else _narrow_aggs(rnd, rnd.randint(0 if i > 2 else 1, 3))
    node = aggregate(a, keys, aggs, key_exprs)
    return _finish(node, [t], r, rnd, False, "n=%d keys=%s" % (n, keys))


def r_group_wide(seed, i, rnd, r):
    """5 to 16 accumulators over 1 to 8 argument columns.  case 0: nine over a few groups (LDS bins); case 1: sixteen over more groups than the 224 bins
    of a tile (global atomics); case 2: MIN / MAX of UInt64 values either side of 2^63, SUM of an Int64 column that wraps; others: random lists,
    group counts either side of 448 / 224"""
    n = size(seed, i, rnd, [700, 4097, 8193] if i < 3 else SIZES)
    groups = {0: 37, 1: 3000}.get(i, rnd.choice([1, 200, 223, 225, 447, 449, 3000]))
    a, t = _one_table("a", n, r, rnd, style="dense", card=groups, nulls={"u": 0.02} if i == 2 else None, key_nulls=rnd.choice([0.0, 0.02]))
    t["a_w"] = with_nulls([2**62 + int(x) for x in r.integers(0, 1000, n)], 0.02, r)
    cols = table_cols("a") + [("a_w", "Int64")]
    a = scan(cols)
    menu = [("count", None), ("count", "a_f"), ("count", "a_s"), ("sum", "a_v"), ("sum", "a_i"), ("avg", "a_v"), ("avg", "a_i"), ("min", "a_f"), ("max", "a_f"),
            ("min", "a_u"), ("max", "a_u"), ("min", "a_t"), ("max", "a_t"), ("min", "a_l"), ("max", "a_i"), ("sum", "a_w"), ("sum", "a_g")]
    if i == 2:
        aggs = [("min", "a_u"), ("max", "a_u"), ("sum", "a_w"), ("count", "a_u"), ("count", None)]
    else:
        want = 9 if i == 0 else 16 if i == 1 else rnd.randint(5, 16)
        aggs, acc = [], 0
        while acc < want:
            f = rnd.choice(menu)
            if acc + (2 if f[0] == "avg" else 1) <= want:
                aggs.append(f)
                acc += 2 if f[0] == "avg" else 1
    keys = ["a_k"] if i < 3 else rnd.choice([["a_k"], ["a_l"], ["a_k", "a_s2"], ["a_s"]])
    node = aggregate(a, keys, aggs)
    return _finish(node, [t], r, rnd, False, "n=%d groups=%d aggs=%d keys=%s" % (n, groups, len(aggs), keys))


def r_distinct_count(seed, i, rnd, r):
    """1 to 4 distinct counts beside other aggregates.  case 0: ungrouped; case 1: grouped by a dense key, arguments with NULLs; case 2: a Utf8
    argument and a Utf8 key; others: random"""
    n = size(seed, i, rnd, [65, 700, 4097, 8193] if i < 3 else SIZES)
    a, t = _one_table("a", n, r, rnd, card=rnd.choice([7, 300, 2049]), nulls={"k": 0.3, "s": 0.3, "l": 0.02} if i in (1, 2) else None,
                      key_nulls=None if i in (1, 2) else rnd.choice([0.0, 0.3]))
    args = ["a_k", "a_l", "a_u", "a_t", "a_s", "a_s2", "a_i"]
    if i == 0:
        keys, aggs = [], [("dc", "a_k"), ("count", None), ("dc", "a_s2")]
    elif i == 1:
        keys, aggs = ["a_g"], [("dc", "a_k"), ("sum", "a_v"), ("dc", "a_l")]
    elif i == 2:
        keys, aggs = ["a_s2"], [("dc", "a_s"), ("count", "a_s")]
    else:
        keys = rnd.choice([[], ["a_g"], ["a_k"], ["a_s2", "a_g"]])
        aggs = [("dc", rnd.choice(args)) for _ in range(rnd.randint(1, 4))] + _narrow_aggs(rnd, rnd.randint(0, 2))
        if not keys:                                             # (an ungrouped COUNT takes no Utf8 column)
            aggs = [("count", None) if f == ("count", "a_s") else f for f in aggs]
        rnd.shuffle(aggs)
    node = aggregate(a, keys, aggs)
    return _finish(node, [t], r, rnd, False, "n=%d keys=%s aggs=%s" % (n, keys, aggs))


def r_global_agg(seed, i, rnd, r):
    """ungrouped lists of up to 8 accumulators.  case 0: over the scan; case 1: directly over a filter; case 2: over a column that is all NULL and
    over no rows at all (SUM of nothing); others: random, a Partial alone once"""
    n = 0 if (i == 2 and seed % 2) else size(seed, i, rnd)
    a, t = _one_table("a", n, r, rnd, nulls={"v": 1.0, "f": 1.0} if i == 2 else None)
    if i == 2:
        aggs = [("sum", "a_v"), ("count", "a_v"), ("min", "a_f"), ("avg", "a_i"), ("count", None), ("sum", "a_i")]
    else:
        aggs, acc = [], 0
        want = rnd.randint(1, 8)
        while acc < want:
            f = rnd.choice([("count", None), ("count", "a_f"), ("sum", "a_v"), ("sum", "a_i"), ("avg", "a_v"), ("min", "a_f"), ("max", "a_u"), ("min", "a_t"),
                            ("max", "a_l"), ("min", "a_u")])
            if acc + (2 if f[0] == "avg" else 1) <= want:
                aggs.append(f)
                acc += 2 if f[0] == "avg" else 1
    inp = a
    if i == 1 or (i > 2 and rnd.random() < 0.5):
        inp = filt(a, Exprs(a, "a", rnd).boolean(2))
    node = aggregate(inp, [], aggs, single="Partial" if i == 5 else None)
    return _finish(node, [t], r, rnd, False, "n=%d aggs=%s" % (n, aggs))


def _join_sides(seed, i, rnd, r, semi):
    """(build table, probe table, key column, note).  The build side (the inner join's LEFT, a semi join's RIGHT) holds every key at most three times,
    so that no result exceeds about 10^5 rows.  case 0: a build side of at most kTinyBuild rows (one workgroup); case 1: both sides above it, unique
    dense build keys; case 2: dense build keys with repeats -- a third of the keys twice, or ONE key on half of the build rows (hot) or on all of them
    (constant), which the probe side then names five times at the most; a semi join's case 2 is hot, constant or, in odd seeds, an EMPTY right side;
    case 3: unique sparse Int64 keys; case 4: sparse with repeats; case 5: composite.  Dense Int32 / Int64 keys sit at 0 or within 20 000 of their
    type's minimum or maximum, UInt64 keys around 2^63."""
    nb = rnd.choice([1, 300, 4096]) if i == 0 else rnd.choice([4097, 9000])
    npr = size(seed, i, rnd, [700, 4097, 8193] if i == 0 else [8191, 8193])
    bstyle = "repeat" if i in (2, 4, 5) else "unique"
    if i == 2:
        bstyle = (["constant", "empty", "hot", "empty"] if semi else ["repeat", "constant", "hot", "repeat"])[seed % 4]
    if bstyle == "empty":
        nb = 0                                                   # an empty right side (case 1 keeps the bitmap in every seed)
    # (NULL keys never reach the join: the one-workgroup kernels take whatever has at most kTinyBuild VALID keys on its smaller side, so a side of
    # 4097 rows is above the threshold only without NULL keys)
    null_choices = [0.0] if nb == 4097 else [0.0, 0.02, 0.3]
    dense = i in (0, 1, 2, 5)
    uniq = [int(x) for x in r.permutation(max(nb, 1) * (2 if dense else 1))[:nb]]
    if not dense:
        uniq = [int(x) for x in set(r.integers(-2**62, 2**62, nb * 2).tolist())][:nb]
        nb = len(uniq)
    hot_key = None
    if bstyle in ("hot", "constant") and nb > 3:
        hot_key = uniq[-1]
        uniq = [hot_key if (bstyle == "constant" or k % 2) else v for k, v in enumerate(uniq)]
    elif bstyle == "repeat" and nb > 3:
        third = nb // 3
        uniq[:third] = uniq[third:2 * third]                     # a third of the keys twice
    bp, pp = ("b", "a") if semi else ("a", "b")
    build = make_table(bp, nb, r, rnd, style="dense", card=50, key_nulls=rnd.choice([0.0, 0.02]))
    kc = "l" if not dense else rnd.choice(["k", "l"]) if i != 0 else rnd.choice(["k", "l", "u", "t"])
    mask = with_nulls([1] * nb, rnd.choice(null_choices), r)
    lo_k, hi_k = _RANGE[{"k": "Int32", "l": "Int64", "u": "UInt64", "t": "Int64"}[kc]]
    off = 2**63 - 100 if kc == "u" else 0 if (not dense or kc == "t") else rnd.choice([0, hi_k - 20_000, lo_k + 10])
    build[bp + "_" + kc] = [None if m is None else v + off for v, m in zip(uniq, mask)]
    probe = make_table(pp, npr, r, rnd, style="dense", card=50, key_nulls=rnd.choice([0.0, 0.02]))
    pool = [v for v in uniq if v != hot_key] + ([int(x) for x in r.integers(-2**62, 2**62, 50)] if not dense else list(range(-5, 0)))
    pstyle = rnd.choice(["any", "any", "hot", "constant"])
    if pstyle == "constant":
        pk = [pool[0]] * npr
    else:
        pk = [pool[int(x)] for x in r.integers(0, len(pool), npr)]
        if pstyle == "hot":
            pk = [pool[0] if h else v for v, h in zip(pk, r.random(npr) < 0.5)]
    if hot_key is not None:
        for at in r.integers(0, npr, 5):
            pk[int(at)] = hot_key
    pm = with_nulls([1] * npr, rnd.choice([0.0, 0.02, 0.3]), r)
    probe[pp + "_" + kc] = [None if m is None else v + off for v, m in zip(pk, pm)]
    if i == 5:      # the second key column: a Utf8 column of few values on both sides
        build[bp + "_s2"] = [None if k % 11 == 3 else WORDS[k % 3] for k in range(nb)]
        probe[pp + "_s2"] = [None if k % 13 == 3 else WORDS[k % 4] for k in range(npr)]
    return build, probe, kc, "build=%d (%s) probe=%d key=%s offset=%d probe_style=%s" % (nb, bstyle, npr, kc, off, pstyle)


def r_join_inner(seed, i, rnd, r):
    """see _join_sides; a filter on either side, an aggregate or a sort on top, at random"""
    build, probe, kc, note = _join_sides(seed, i, rnd, r, False)
    a, b = scan(table_cols("a")), scan(table_cols("b"))
    names_a, names_b = ["a_" + kc, "a_id", "a_v", "a_s2", "a_f"], ["b_" + kc, "b_id", "b_i", "b_s2", "b_t"]
    la, lb = keep(a, names_a), keep(b, names_b)
    if rnd.random() < 0.3 and len(build["a_id"]) > 5000:        # (a filter that takes a 4097-row side to 4096 rows takes the join to one workgroup)
        la = filt(la, binop(la.c("a_id"), "NotEq", lit("Int64", 3)))
    if rnd.random() < 0.3:
        lb = filt(lb, binop(lb.c("b_id"), "GtEq", lit("Int64", 2)))
    on = [("a_" + kc, "b_" + kc)] + ([("a_s2", "b_s2")] if i == 5 else [])
    node = join("Inner", la, lb, on)
    top = rnd.choice(["none", "none", "agg", "sort"])
    ordered = False
    if top == "agg":
        node = aggregate(node, ["a_" + kc], [("count", None), ("sum", "b_i"), ("min", "a_f")])
    elif top == "sort":
        node = sort(node, [("b_s2", rnd.random() < 0.5, rnd.random() < 0.5), ("a_id", False, False), ("b_id", True, False)])
        ordered = True
    return _finish(node, [build, probe], r, rnd, ordered, note + " top=" + top)


def r_join_semi_anti(seed, i, rnd, r):
    """see _join_sides (the build side is the RIGHT input: a set); Semi and Anti alternate with seed and case, the two empty right sides (case 2 of
    seeds 1 and 3) take one each"""
    build, probe, kc, note = _join_sides(seed, i, rnd, r, True)
    jt = "Semi" if (seed + i + (seed // 2 if i == 2 else 0)) % 2 == 0 else "Anti"
    a, b = scan(table_cols("a")), scan(table_cols("b"))
    la, lb = keep(a, ["a_" + kc, "a_id", "a_s2", "a_v"]), keep(b, ["b_" + kc, "b_s2"])
    if rnd.random() < 0.3 and len(build["b_s2"]) > 5000:
        lb = filt(lb, {"physical_expr": "is_not_null_expr", "arg": lb.c("b_s2")})
    on = [("a_" + kc, "b_" + kc)] + ([("a_s2", "b_s2")] if i == 5 else [])
    node = join(jt, la, lb, on)
    top = rnd.choice(["none", "none", "agg"])
    if top == "agg":
        node = aggregate(node, ["a_s2"], [("count", None), ("sum", "a_v")])
    return _finish(node, [probe, build], r, rnd, False, "%s %s top=%s" % (jt, note, top))


def r_sort_limit(seed, i, rnd, r):
    """1 to 4 sort keys, ASC / DESC x nulls first / last, the row's number as the last key.  case 0: one Int32 key of a few bits; case 1: ONE Int64
    key without NULLs, DESC (relops.hip: the only way to sort_int_digit_kernel); case 2: a Utf8 key with shared prefixes, then a Float64 key; case 3: a limit over the sort; others: random"""
    n = size(seed, i, rnd, [65, 700, 4095, 4097, 8193] if i < 4 else SIZES)
    style = {0: "dense", 1: "sparse"}.get(i, rnd.choice(KEY_STYLES))
    a, t = _one_table("a", n, r, rnd, style=style, card={0: 3}.get(i, rnd.choice([2, 300, 5000])), key_nulls=rnd.choice([0.02, 0.3]), nulls={"f": 0.3, "u": 0.02})
    opt = lambda: (rnd.random() < 0.5, rnd.random() < 0.5)
    if i == 0:
        keys = [("a_k",) + opt()]
    elif i == 1:
        keys = []                                                # the row's number alone, DESC: ONE integer key without NULLs (sort_int_digit_kernel)
    elif i == 2:
        keys = [("a_s",) + opt(), ("a_f",) + opt()]
    else:
        keys = [(c,) + opt() for c in rnd.sample(["a_k", "a_l", "a_g", "a_u", "a_t", "a_f", "a_s", "a_s2", "a_i"], rnd.randint(1, 3))]
    keys.append(("a_id", i == 1 or rnd.random() < 0.3, False))
    names = sorted({k for k, _, _ in keys} | {"a_id", "a_v"})
    if i % 2:                                                    # the leaf's own projection in place of a ProjectionExec over it
        leaf = scan(table_cols("a"), projection=sorted(a.cols.index((c, a.ty(c))) for c in names))
    else:
        leaf = keep(a, names)
    node = sort(leaf, keys)
    if i == 3 or (i > 3 and rnd.random() < 0.4):
        node = limit(node, rnd.choice([0, 1, 50, 5000]))
    return _finish(node, [t], r, rnd, True, "n=%d keys=%s" % (n, keys))


def r_window(seed, i, rnd, r):
    """the planner's sort under the node.  case 0: ROW_NUMBER and two aggregates, partitions of a few rows; case 1: one partition longer than a tile,
    peers on the ORDER BY key; case 2: NULL partition and order keys; case 3: FOUR PARTITION BY and FOUR ORDER BY columns (window.hip takes at most four of
    each, kWinMaxKeys = 8 key columns), the columns rewritten so that partitions and peer groups still hold several rows; others: 1 to 4 PARTITION BY
    columns of (k, g, l, t) and 0 to 4 ORDER BY columns of (u, i, v, f)"""
    n = size(seed, i, rnd, [65, 700, 4097, 8193] if i < 4 else SIZES)
    a, t = _one_table("a", n, r, rnd, style="constant" if i == 1 else "dense", card=7 if i == 3 else rnd.choice([7, 300]), key_nulls=0.3 if i == 2 else rnd.choice([0.0, 0.02]),
                      groups=rnd.choice([5, 37]))
    if i == 0:
        part, order = ["a_k"], ["a_g"]
    elif i == 1:
        part, order = ["a_k"], ["a_g"]
    elif i == 2:
        part, order = ["a_k"], ["a_l"]
    else:
        pmenu, omenu = ["a_k", "a_g", "a_l", "a_t"], ["a_u", "a_i", "a_v", "a_f"]
        if i == 3 or rnd.random() < 0.5:     # l follows k and t follows g, the order columns take two or three values: several rows per partition and peer group
            t["a_l"] = [None if v is None else v * 10**10 for v in t["a_k"]]
            t["a_t"] = [None if v is None else v * 1000 - 5 for v in t["a_g"]]
            t["a_i"] = with_nulls([int(x) for x in r.integers(-1, 2, n)], 0.02, r)
            t["a_v"] = with_nulls([int(x) for x in r.integers(0, 2, n)], 0.02, r)
            t["a_f"] = [int(x) / 4 + 0.25 for x in r.integers(0, 3, n)]
        part = list(pmenu) if i == 3 else rnd.sample(pmenu, rnd.randint(1, 4))
        order = list(omenu) if i == 3 else rnd.sample(omenu, rnd.randint(0, 4))
    fns = [("count", None), ("count", "a_f"), ("sum", "a_v"), ("sum", "a_i"), ("min", "a_f"), ("max", "a_u"), ("avg", "a_v"), ("max", "a_t"), ("min", "a_i")]
    entries = [("row_number", None, part, [])] if i in (0, 2) or rnd.random() < 0.5 else []
    entries += [(f, arg, part, order if rnd.random() < 0.7 or i in (1, 2) else []) for f, arg in rnd.sample(fns, rnd.randint(2, 4))]
    # (ROW_NUMBER numbers the rows of a partition as they arrive: the row's number as the sort's last key makes that order the same everywhere)
    srt = sort(a, [(p, False, False) for p in part] + [(o, False, False) for o in order] + ([("a_id", False, False)] if entries[0][0] == "row_number" else []))
    node = window(srt, entries)
    names = [c for c, _ in node.cols[:len(entries)]] + ["a_id"] + part + order
    node = keep(node, list(dict.fromkeys(names)))
    return _finish(node, [t], r, rnd, False, "n=%d part=%s order=%s entries=%s" % (n, part, order, [e[:2] for e in entries]))


def r_cross(seed, i, rnd, r):
    """case 0: a one-row right side -- an ungrouped aggregate -- under a filter that compares with it; case 1: two small sides with Utf8 columns; case
    2: ROW_NUMBER over the pairs of a constant partition key (the pair order); others: small sides under a filter with a scalar function or a
    projection"""
    nl = size(seed, i, rnd, [1, 63, 65, 700] if i else [65, 700, 4097, 8193])
    nr = rnd.choice([1, 2, 7, 64, 65]) if i else 1
    if nl > 700 and i:
        nr = rnd.choice([1, 2])
    lt = make_table("a", nl, r, rnd)
    rt = make_table("b", nr, r, rnd)
    a, b = keep(scan(table_cols("a")), ["a_id", "a_v", "a_s2", "a_f", "a_g"]), keep(scan(table_cols("b")), ["b_id", "b_s", "b_i", "b_t"])
    if i == 0:
        bb = aggregate(scan(table_cols("b")), [], [("avg", "b_v"), ("max", "b_i")])
        node = cross(a, bb)
        node = filt(node, binop(cast(node.c("a_v"), "Float64"), "Gt", node.c(bb.cols[0][0])))
    elif i == 2:
        node = cross(a, b)
        node = proj(node, [(node.c(n), n, node.ty(n)) for n in ["a_id", "b_id"]] + [(binop(node.c("a_id"), "Multiply", lit("Int64", 0)), "one", "Int64")])
        node = keep(window(node, [("row_number", None, ["one"], [])]), ["w0:rn", "a_id", "b_id"])
    else:
        node = cross(a, b)
        how = rnd.choice(["filter", "project", "none"])
        if how == "filter":
            node = filt(node, binop(fn("abs", "Float64", node.c("a_f")), "Gt", cast(node.c("b_i"), "Float64")))
        elif how == "project":
            node = proj(node, [(node.c("a_id"), "a_id", "Int64"), (node.c("b_s"), "b_s", "Utf8"), (binop(node.c("a_v"), "Plus", cast(node.c("b_i"), "Int64")), "sum", "Int64")])
    return _finish(node, [lt, rt], r, rnd, False, "left=%d right=%d" % (nl, nr))


def r_mixed(seed, i, rnd, r):
    """trees of 3 to 6 operators: 0 join under aggregate under sort; 1 window over a join; 2 semi join over a text-keyed aggregate; 3 the same
    sub-tree named twice (an aggregate joined with its own maximum); 4 a sort over an aggregate whose key column is all NULL; 5 a cross join
    feeding a filter with a scalar function under an aggregate"""
    n = size(seed, i, rnd, [65, 700, 4097, 8193])
    a = scan(table_cols("a"))
    ta = make_table("a", n, r, rnd, style="dense", card=rnd.choice([7, 300]), nulls={"k": 1.0} if i == 4 else {"k": 0.02, "v": 0.02})
    tables, ordered = [ta], False
    if i in (0, 1):
        nb = rnd.choice([300, 4097])
        tb = make_table("b", nb, r, rnd, style="unique", key_nulls=0.02)
        tb["b_k"] = with_nulls([int(x) - 3 for x in r.permutation(nb)], 0.02, r)
        tables.insert(0, tb)                                     # (the join's LEFT leaf comes first)
        j = join("Inner", keep(scan(table_cols("b")), ["b_k", "b_s2", "b_i"]), keep(a, ["a_k", "a_id", "a_v", "a_g"]), [("b_k", "a_k")])
        if i == 0:
            node = sort(aggregate(j, ["b_s2"], [("count", None), ("sum", "a_v"), ("max", "b_i")]), [("b_s2", rnd.random() < 0.5, rnd.random() < 0.5)])
            ordered = True
        else:
            srt = sort(j, [("a_g", False, False), ("a_v", False, False)])
            node = keep(window(srt, [("row_number", None, ["a_g"], []), ("sum", "b_i", ["a_g"], ["a_v"]), ("count", None, ["a_g"], [])]),
                        ["w0:rn", "w1:SUM(b_i)", "w2:COUNT(UInt8(1))", "a_id", "a_g", "a_v"])
            node = keep(node, ["w1:SUM(b_i)", "w2:COUNT(UInt8(1))", "a_id", "a_g", "a_v"])     # (row numbers among equal a_v are the sort's business)
    elif i == 2:
        label = case_([(binop(a.c("a_g"), "Lt", lit("Int32", 2)), lit("Utf8", "low")), (binop(a.c("a_g"), "Lt", lit("Int32", 4)), a.c("a_s2"))], lit("Utf8", "high"))
        g = aggregate(proj(a, [(label, "label", "Utf8"), (a.c("a_v"), "a_v", "Int64")]), ["label"], [("count", None), ("sum", "a_v")])
        tb = make_table("b", rnd.choice([7, 300]), r, rnd)
        tables.append(tb)
        node = join(rnd.choice(["Semi", "Anti"]), g, keep(scan(table_cols("b")), ["b_s2"]), [("label", "b_s2")])
    elif i == 3:
        counts = lambda: aggregate(keep(a, ["a_g"]), ["a_g"], [("count", None)])
        c1, c2 = counts(), counts()
        mx = aggregate(c2, [], [("max", c2.cols[1][0])])
        node = join("Inner", c1, mx, [(c1.cols[1][0], mx.cols[0][0])])
    elif i == 4:
        node = sort(aggregate(a, ["a_k", "a_g"], [("count", None), ("min", "a_f")]), [("a_k", rnd.random() < 0.5, rnd.random() < 0.5), ("a_g", True, False)])
        ordered = True
    else:
        tb = make_table("b", rnd.choice([1, 7]), r, rnd)
        tables.append(tb)
        ta2 = {k: v[:700] for k, v in ta.items()}
        tables[0] = ta2
        node = cross(keep(a, ["a_f", "a_g", "a_v"]), keep(scan(table_cols("b")), ["b_f", "b_i"]))
        node = filt(node, binop(fn("floor", "Float64", node.c("a_f")), "GtEq", fn("ceil", "Float64", node.c("b_f"))))
        node = aggregate(node, ["a_g"], [("count", None), ("sum", "a_v"), ("min", "b_i")])
    return _finish(node, tables, r, rnd, ordered, "n=%d shape=%d" % (n, i))


def r_errors(seed, i, rnd, r):
    """an otherwise valid projection with exactly ONE row that fails the call, at a random position or at a tile boundary: 0 an Int32 zero divisor, 1
    an Int64 zero modulus, 2 a Float64 zero divisor, 3 INT_MIN / -1, 4 a CAST that does not fit, 5 a zero divisor under a filter's predicate"""
    n = size(seed, i, rnd, [1, 65, 700, 8192, 8193])
    a, t = _one_table("a", n, r, rnd, nulls={"g": 0.0, "v": 0.0, "f": 0.0, "i": 0.0, "l": 0.0})
    at = rnd.choice([0, n - 1, rnd.randrange(n)] + ([8191, 8192] if n > 8192 else []))
    t["a_g"] = [x + 1 for x in t["a_g"]]
    t["a_v"] = [x if x else 1 for x in t["a_v"]]
    t["a_i"] = [x if x not in (0, -2**31) else 1 for x in t["a_i"]]
    one = lit("Int32", 1)
    if i in (0, 5):
        t["a_g"][at] = 0
        e, ty = binop(a.c("a_i"), "Divide", a.c("a_g")), "Int32"
    elif i == 1:
        t["a_v"][at] = 0
        e, ty = binop(a.c("a_id"), "Modulo", a.c("a_v")), "Int64"
    elif i == 2:
        t["a_f"][at] = rnd.choice([0.0, -0.0])
        e, ty = binop(lit("Float64", 1.0), "Divide", a.c("a_f")), "Float64"
    elif i == 3:
        t["a_i"][at] = -2**31
        e, ty = binop(a.c("a_i"), "Divide", binop(binop(a.c("a_g"), "Multiply", lit("Int32", 0)), "Minus", one)), "Int32"
    else:
        t["a_l"] = [int(x) % 1000 for x in range(n)]
        t["a_l"][at] = 2**31
        e, ty = cast(a.c("a_l"), "Int32"), "Int32"
    if i == 5:
        node = filt(a, binop(e, "Gt", lit("Int32", 0)))
    else:
        node = proj(a, [(a.c("a_id"), "a_id", "Int64"), (e, "e", ty)])
    return _finish(node, [t], r, rnd, False, "n=%d at=%d" % (n, at))


# ------------------------------------------------------------------ UNION ALL and the text casts (their own generators: the recipes above stay as they were)
def union(inputs):
    """UNION ALL of Nodes whose columns agree in type by position; the names are input 0's"""
    first = inputs[0]
    assert all([t for _, t in x.cols] == [t for _, t in first.cols] for x in inputs), [x.cols for x in inputs]
    return Node({"execution_plan": "union_exec", "inputs": [x.plan for x in inputs], "schema": schema(first.cols)}, first.cols)


def ordered_union(plan):
    """a union at the root over scans, filters and projections (unions of such included) has a defined row order: A-U2, and a filter keeps its
    input's order"""
    def plain(node):
        kind = node.get("execution_plan")
        if kind == "memory_exec":
            return True
        if kind == "union_exec":
            return all(plain(x) for x in node["inputs"])
        return kind in ("filter_exec", "projection_exec", "coalesce_batches_exec") and plain(node["input"])
    return plan.get("execution_plan") == "union_exec" and all(plain(x) for x in plan["inputs"])


UNION_ROWS = [0, 1, 3, 5, 7, 4097]


def _renamed(inp, names):
    return proj(inp, [(inp.c(old), new, t) for (old, t), new in zip(inp.cols, names)])


def _id_mod(node, name, m, j):
    return binop(binop(node.c(name), "Modulo", lit("Int64", m)), "Eq", lit("Int64", j))


def r_union(seed, i, rnd, r):
    """case 0: two plain scans of two relations, every column, one relation without a NULL anywhere, row counts of UNION_ROWS (seams at every
    misalignment); case 1: two filters over ONE relation that read different columns of it; case 2: three to five inputs -- one empty, one all NULL,
    one a union itself -- under a sort and a limit; case 3: 17 to 33 small inputs under a GROUP BY on (Int32, Utf8); case 4: a union as one side of an
    Inner / Semi / Anti join; case 5: UNION DISTINCT (a key-only aggregate) over a projection with a literal and an id as text beside a join or an
    aggregate.  Cases 0 and 1 are ordered: the root is a union over scans, filters and projections."""
    a, b = scan(table_cols("a")), scan(table_cols("b"))
    if i == 0:
        na, nb = rnd.choice(UNION_ROWS), rnd.choice(UNION_ROWS)
        plain = rnd.choice(["a", "b"])
        every = {c: 0.0 for c, _ in COLS}
        ta = make_table("a", na, r, rnd, nulls=every if plain == "a" else {"s": 0.3, "k": 0.02})
        tb = make_table("b", nb, r, rnd, nulls=every if plain == "b" else {"s": 0.3, "k": 0.02})
        return _finish(union([a, b]), [ta, tb], r, rnd, True, "rows=%d+%d no NULL in %s" % (na, nb, plain))
    if i == 1:
        n = size(seed, i, rnd, SIZES[1:])
        ta = make_table("a", n, r, rnd, nulls={"k": 0.02, "i": 0.3, "s": 0.3, "s2": 0.0})
        x = Exprs(a, "a", rnd)
        one = proj(filt(a, x.simple(1)), [(a.c("a_id"), "id", "Int64"), (a.c("a_k"), "n", "Int32"), (a.c("a_s"), "w", "Utf8")])
        src = keep(a, ["a_v", "a_i", "a_s2"])
        two = filt(src, binop(src.c("a_i"), rnd.choice(["Lt", "GtEq"]), lit("Int32", rnd.choice([0, 2**30]))))
        return _finish(union([one, two]), [ta], r, rnd, True, "n=%d one relation twice" % n)
    if i == 2:
        n = size(seed, i, rnd)
        count = rnd.randint(3, 5)
        names = ["k", "s", "u", "n"]
        tables, parts = [], []
        roles = ["empty", "null", "nested"] + ["plain"] * (count - 3)
        rnd.shuffle(roles)
        for j, role in enumerate(roles):
            p = "abcdefg"[len(tables)]
            rows = 0 if role == "empty" else n if j == 0 or role == "nested" else rnd.choice([1, 65, 700])
            t = make_table(p, rows, r, rnd, nulls={"k": 1.0, "s": 1.0, "u": 1.0, "l": 1.0} if role == "null" else {"k": 0.02, "s": 0.3, "u": 0.0})
            s = scan(table_cols(p))
            node = _renamed(keep(s, [p + "_k", p + "_s", p + "_u", p + ("_l" if role == "null" else "_id")]), names)
            if role == "nested":
                q = "abcdefg"[len(tables) + 1]
                t2 = make_table(q, rnd.choice([1, 7, 300]), r, rnd)
                s2 = scan(table_cols(q))
                other = _renamed(keep(s2, [q + "_g", q + "_s2", q + "_u", q + "_v"]), names)
                swap = rnd.random() < 0.5
                node = union([other, node] if swap else [node, other])
                tables += [t2, t] if swap else [t, t2]                # (tables in leaf order)
            else:
                tables.append(t)
            parts.append(node)
        u = union(parts)
        keys = [(c, rnd.random() < 0.5, rnd.random() < 0.5) for c in rnd.sample(names, 4)]      # every column is a key: only identical rows tie
        node = limit(sort(u, keys), [5000, 50, 100_000, 1][seed % 4])
        return _finish(node, tables, r, rnd, True, "n=%d inputs=%s" % (n, roles))
    if i == 3:
        n = size(seed, i, rnd, [65, 700, 4097])
        count, m = rnd.randint(17, 33), rnd.choice([3, 7])
        ta = make_table("a", n, r, rnd, style="dense", card=rnd.choice([7, 300]), nulls={"s2": 0.3, "v": 0.02}, key_nulls=0.02)
        tb = make_table("b", rnd.choice([1, 65, 300]), r, rnd, style="dense", card=7, key_nulls=0.3)
        parts = []
        for j in range(count):
            if j % 8 == 5:
                parts.append(keep(b, ["b_k", "b_s2", "b_v", "b_id"]))                # a plain input among the row lists
            else:
                src = keep(a, ["a_k", "a_s2", "a_v", "a_id"])
                parts.append(filt(src, _id_mod(src, "a_id", m, j % m)))
        node = aggregate(union(parts), ["a_k", "a_s2"], [("count", None), ("sum", "a_v"), ("max", "a_id")])
        return _finish(node, [ta, tb], r, rnd, False, "n=%d inputs=%d modulus=%d" % (n, count, m))
    if i == 4:
        n = size(seed, i, rnd, [700, 4097, 8193])
        nb = rnd.choice(BUILD_SIZES)
        jt = ["Inner", "Semi", "Anti", "Inner"][seed % 4]
        ta = make_table("a", n, r, rnd, style="dense", card=nb, key_nulls=0.02, nulls={"s2": 0.3})
        tb = make_table("b", rnd.choice([1, 300, 4097]), r, rnd, style="dense", card=nb, key_nulls=0.3)
        tc = make_table("c", nb, r, rnd, key_nulls=0.0)
        tc["c_k"] = with_nulls([int(v) - nb // 4 for v in r.permutation(nb)], rnd.choice([0.0, 0.02]), r)
        first = keep(a, ["a_k", "a_id", "a_s2", "a_v"])
        u = union([filt(first, _id_mod(first, "a_id", 2, 0)), keep(b, ["b_k", "b_id", "b_s2", "b_v"]), filt(first, _id_mod(first, "a_id", 2, 1))])
        build = keep(scan(table_cols("c")), ["c_k", "c_s", "c_id"])
        if jt == "Inner":
            node, tables = join("Inner", build, u, [("c_k", "a_k")]), [tc, ta, tb]
        else:
            node, tables = join(jt, u, build, [("a_k", "c_k")]), [ta, tb, tc]
        if rnd.random() < 0.4:
            node = aggregate(node, ["a_s2"], [("count", None), ("sum", "a_v")])
        return _finish(node, tables, r, rnd, False, "n=%d build=%d %s" % (n, nb, jt))
    n = size(seed, i, rnd, SIZES[1:])
    ta = make_table("a", n, r, rnd, groups=37, nulls={"g": 0.02})
    tb = make_table("b", rnd.choice([65, 700, 4097]), r, rnd, style="dense", card=50, key_nulls=0.02, nulls={"s2": 0.3})
    one = proj(a, [(lit("Utf8", rnd.choice(["bid", "", "sixteen_bytes_pfx"])), "kind", "Utf8"), (cast(a.c("a_g"), "Utf8"), "who", "Utf8")])
    tables = [ta, tb]
    if rnd.random() < 0.5:
        two = aggregate(b, ["b_s2", "b_s"], [])
    else:
        tc = make_table("c", 300, r, rnd)
        tc["c_k"] = [int(v) - 5 for v in r.permutation(300)]
        j = join("Inner", keep(scan(table_cols("c")), ["c_k", "c_s2"]), keep(b, ["b_k", "b_s"]), [("c_k", "b_k")])
        two = keep(j, ["c_s2", "b_s"])
        tables = [ta, tc, tb]
    node = aggregate(union([one, two]), ["kind", "who"], [])
    return _finish(node, tables, r, rnd, False, "n=%d second=%s" % (n, two.plan["execution_plan"]))


TS_MIN = -62167219200000                     # 0000-01-01 00:00:00.000
TS_MAX = 253402300799999                     # 9999-12-31 23:59:59.999
_DAY = 86_400_000


def number_pools():
    """the directed values of the cast to text: integers of every digit count from 1 to 20 with both ends of every type and UInt64 at and above
    2^63; timestamps either side of 1970 with and without a millisecond part, the first and last millisecond of the years 0000 and 9999"""
    i32 = [0, -2**31, 2**31 - 1] + [s * (10**d + e) for d in range(10) for s in (1, -1) for e in (0, -1)]
    i64 = [-2**63, 2**63 - 1] + [s * (10**d + e) for d in range(19) for s in (1, -1) for e in (0, -1)]
    u64 = [0, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1, 10**19, 10**19 - 1] + [10**d + e for d in range(20) for e in (0, -1)]
    ts = [0, 1, -1, 999, 1000, -1000, -999, -1001, 86_399_999, -86_400_000, 1_436_951_287_123, 1_436_951_287_000, -1_436_951_287_123, -1_436_951_287_000,
          TS_MIN, TS_MIN + 1, TS_MIN + 366 * _DAY - 1, TS_MIN + 366 * _DAY, TS_MAX, TS_MAX - 999, TS_MAX + 1 - 365 * _DAY, TS_MAX - 365 * _DAY]
    return {"i": [v for v in i32 if -2**31 <= v < 2**31], "l": i64, "u": [v for v in u64 if v >= 0], "t": ts}


def pooled(pool, n, r, share):
    """n values: the pool in order first (as far as n reaches), then draws from it; NULL with `share`"""
    vals = [pool[k] if k < len(pool) else pool[int(x)] for k, x in enumerate(r.integers(0, len(pool), n))]
    return with_nulls(vals, share, r)


def r_cast_text(seed, i, rnd, r):
    """CAST(number | timestamp AS Utf8).  case 0: projected casts of the Int32, Int64, UInt64 and Timestamp columns over number_pools(); case 1:
    try_cast_expr of timestamps, some outside the years 0000 to 9999 (NULL); case 2: the cast of a computed expression, as a branch of a text CASE
    and under left / right / split_part / trims; case 3: as a GROUP BY key and as the argument of COUNT and COUNT(DISTINCT); case 4: as an ORDER BY
    key with a_id as the last key; case 5: beside a Utf8 column in a union branch and under a filter, below a join"""
    n = size(seed, i, rnd, [700, 1025, 4097, 8193] if i < 2 else [65, 700, 4097, 8193] if i < 4 else SIZES)      # (cases 0 and 1: every value of a pool)
    a = scan(table_cols("a"))
    t = make_table("a", n, r, rnd, style="dense", card=300, groups=37, nulls={"g": 0.02, "k": 0.02, "v": 0.02, "f": 0.02, "s": 0.3, "s2": 0.02})
    pools = number_pools()
    share = rnd.choice([0.02, 0.3])
    if i in (0, 1):
        for c in "ilut":
            t["a_" + c] = pooled(pools[c] + ([TS_MAX + 1, TS_MIN - 1, 2**62, -2**63, 2**63 - 1] if (c == "t" and i == 1) else []), n, r, share)
    x = Exprs(a, "a", rnd)
    tables, ordered = [t], False
    if i == 0:
        node = proj(a, [(x.c("id"), "a_id", "Int64")] + [(cast(x.c(c), "Utf8"), "x" + c, "Utf8") for c in "ilut"])
    elif i == 1:
        node = proj(a, [(x.c("id"), "a_id", "Int64"), (cast(x.c("t"), "Utf8", safe=True), "xt", "Utf8"), (cast(x.c("u"), "Utf8", safe=True), "xu", "Utf8")])
    elif i == 2:
        day = fn("left", "Utf8", cast(x.c("t"), "Utf8"), lit("Int64", 10))
        es = [cast(x.nl(x.int64(2), "v"), "Utf8"), cast(x.nl(x.int32(2), "i"), "Utf8"), cast(x.ts(1), "Utf8"),
              case_([(x.plain_boolean(), cast(x.c("l"), "Utf8")), (x.plain_boolean(), x.c("s2"))], rnd.choice([None, lit("Utf8", "none"), cast(x.c("g"), "Utf8")])),
              day, fn("right", "Utf8", fn("left", "Utf8", cast(x.c("t"), "Utf8"), lit("Int64", 16)), lit("Int64", 5)),
              fn("split_part", "Utf8", cast(x.c("t"), "Utf8"), lit("Utf8", rnd.choice(["-", ":", " "])), lit("Int64", rnd.randint(1, 3))),
              fn(rnd.choice(["ltrim", "btrim"]), "Utf8", cast(x.c("i"), "Utf8"), lit("Utf8", "-1")), fn("rtrim", "Utf8", cast(x.c("v"), "Utf8"), lit("Utf8", "0"))]
        picked = es[:3] + rnd.sample(es[3:], 3)
        node = proj(a, [(x.c("id"), "a_id", "Int64")] + [(e, "x%d" % k, "Utf8") for k, e in enumerate(picked)])
    elif i == 3:
        key = rnd.choice(["g", "k", "t"])
        if key == "t":
            t["a_t"] = [None if v is None else v // 3_600_000 * 3_600_000 for v in t["a_t"]]
        below = proj(a, [(cast(x.c(key), "Utf8"), "x0", "Utf8"), (cast(x.c("k"), "Utf8"), "x1", "Utf8"), (x.c("v"), "a_v", "Int64")])
        node = aggregate(below, ["x0"], [("count", "x1"), ("dc", "x1"), ("count", None), ("sum", "a_v")])
    elif i == 4:
        key = rnd.choice(["v", "g", "t", "u"])
        below = proj(a, [(x.c("id"), "a_id", "Int64"), (cast(x.c(key), "Utf8"), "x0", "Utf8")])
        node = sort(below, [("x0", rnd.random() < 0.5, rnd.random() < 0.5), ("a_id", False, False)])
        ordered = True
    else:
        b = scan(table_cols("b"))
        tb = make_table("b", rnd.choice([1, 300, 4097]), r, rnd, style="dense", card=300, key_nulls=0.02)
        nc = rnd.choice([300, 4097])
        tc = make_table("c", nc, r, rnd)
        tc["c_k"] = [int(v) - 100 for v in r.permutation(nc)]
        one = proj(a, [(x.c("k"), "k", "Int32"), (cast(x.c("id"), "Utf8"), "who", "Utf8"), (x.c("s"), "w", "Utf8")])
        below = proj(b, [(b.c("b_k"), "b_k", "Int32"), (cast(b.c("b_l"), "Utf8"), "xl", "Utf8"), (b.c("b_s2"), "b_s2", "Utf8")])
        two = filt(below, binop(below.c("b_k"), "GtEq", lit("Int32", rnd.choice([-50, 0, 40]))))
        node = join("Inner", keep(scan(table_cols("c")), ["c_k", "c_s"]), union([one, two]), [("c_k", "k")])
        tables = [tc, t, tb]
    return _finish(node, tables, r, rnd, ordered, "n=%d" % n)


def text_numbers(target, n, rnd, valid=True, bound=None):
    """n texts for a cast to `target` ('Int32' | 'Int64' | 'UInt64' | 'Timestamp'), deterministic in `rnd` (a random.Random), built on
    parse_text_ref's own generators.  valid: every value parses -- zeros in front beyond 24 bytes, a leading '+', '-0' for the signed types and both
    limits among them; otherwise parse_text_ref.EDGES first, then values and their mutations.  bound: integers of magnitude below it only."""
    import parse_text_ref as ptref
    make = ptref._ts_text if target == "Timestamp" else ptref._int_text
    out = []
    if not valid:
        out = list(ptref.EDGES)[:n]
    elif target != "Timestamp" and bound is None:
        lo, hi = ptref.LIMITS[target]
        out = [str(lo), str(hi), "0" * 30 + "7", "+5", "+" + str(hi), "0", "007"] + (["-0", "-" + "0" * 25 + "12", "-000"] if lo < 0 else ["0" * 24 + str(hi)])
        out = out[:n]
    while len(out) < n:
        if bound is not None:
            v = rnd.randrange(-bound + 1, bound)
            s = rnd.choice(["%d", "%d", "%d", "%+d", "%05d", "%030d"]) % v
        else:
            s = make(rnd)
        if not valid and rnd.random() < 0.5:
            s = ptref._mutate(rnd, s)
        if valid and ptref.parse_one(s, target) is None:
            continue
        out.append(s)
    return out


PARSE_COLS = [("a_n", "Utf8"), ("a_m", "Utf8"), ("a_p", "Utf8"), ("a_d", "Utf8"), ("a_q", "Utf8")]


def parse_table(n, r, rnd, valid=True, bound=None):
    """table_cols('a') and PARSE_COLS: a_n / a_m / a_p texts for Int32 / Int64 / UInt64, a_d for Timestamp, a_q `key=<Int32>/<Int64>` for the slices"""
    t = make_table("a", n, r, rnd, groups=5, nulls={"g": 0.02, "k": 0.02, "i": 0.02, "f": 0.02, "t": 0.02, "l": 0.02, "u": 0.02})
    share = rnd.choice([0.0, 0.02, 0.3])
    for name, target in (("a_n", "Int32"), ("a_m", "Int64"), ("a_p", "UInt64"), ("a_d", "Timestamp")):
        t[name] = with_nulls(text_numbers(target, n, rnd, valid, bound if target != "Timestamp" else None), share, r)
    first, second = text_numbers("Int32", n, rnd, True, bound), text_numbers("Int64", n, rnd, True, bound)
    t["a_q"] = with_nulls(["%s=%s/%s" % (WORDS[k % 7], p, q) for k, (p, q) in enumerate(zip(first, second))], share, r)
    return scan(table_cols("a") + PARSE_COLS), t


_PARSE_TARGETS = [("a_n", "Int32"), ("a_m", "Int64"), ("a_p", "UInt64"), ("a_d", "ts")]


def r_parse_text(seed, i, rnd, r):
    """CAST(text AS Int32 / Int64 / UInt64 / Timestamp).  case 0: cast_expr of columns of valid values to each integer target; case 1:
    try_cast_expr over the edge table and mutated values, to all four targets; case 2: the cast of split_part / left chains (the parse reads (begin,
    end) pairs in place); case 3: the cast of a text CASE and of a number cast to Utf8 (the materialised route); case 4: the cast in a filter predicate
    and as the argument of SUM, MIN and MAX, magnitudes below 2^31; case 5: through a projection, as a join key against an Int64 id (Inner and Semi)
    and as a GROUP BY or ORDER BY key"""
    n = size(seed, i, rnd, [700, 1025, 4097, 8193] if i == 1 else [65, 700, 1025, 4097, 8193] if i < 4 else SIZES[2:])      # (case 1: the whole edge table)
    a, t = parse_table(n, r, rnd, valid=i != 1, bound=2**31 if i == 4 else None)
    c = a.c
    tables, ordered = [t], False
    ident = (c("a_id"), "a_id", "Int64")
    if i == 0:
        node = proj(a, [ident] + [(cast(c(name), ty), "v" + name[-1], ty) for name, ty in _PARSE_TARGETS[:3]] + [(cast(c("a_n"), "Int64"), "wide", "Int64")])
    elif i == 1:
        node = proj(a, [ident] + [(cast(c(name), ty, safe=True), "v%d%s" % (k, name[-1]), ty) for k, (_, ty) in enumerate(_PARSE_TARGETS) for name in ("a_n", "a_d")])
    elif i == 2:
        tail = fn("split_part", "Utf8", c("a_q"), lit("Utf8", "/"), lit("Int64", 2))
        mid = fn("split_part", "Utf8", fn("split_part", "Utf8", c("a_q"), lit("Utf8", "="), lit("Int64", 2)), lit("Utf8", "/"), lit("Int64", 1))
        node = proj(a, [ident, (cast(tail, "Int64"), "tail", "Int64"), (cast(mid, "Int32"), "mid", "Int32"),
                        (cast(fn("left", "Utf8", c("a_d"), lit("Int64", 10)), "ts"), "day", "ts"),
                        (cast(fn("right", "Utf8", tail, lit("Int64", rnd.choice([1, 3, 30]))), "UInt64", safe=True), "last", "UInt64"),
                        (cast(fn("left", "Utf8", c("a_m"), lit("Int64", rnd.choice([1, 2, 9]))), "Int32", safe=True), "head", "Int32")])
    elif i == 3:
        x = Exprs(a, "a", rnd)
        label = case_([(x.plain_boolean(), c("a_n")), (x.plain_boolean(), lit("Utf8", rnd.choice(["77", "+0", "none"])))], rnd.choice([None, c("a_m"), cast(c("a_k"), "Utf8")]))
        node = proj(a, [ident, (cast(fn("left", "Utf8", cast(c("a_t"), "Utf8"), lit("Int64", 10)), "ts"), "day", "ts"),
                        (cast(cast(c("a_t"), "Utf8"), "ts"), "again", "ts"), (cast(label, "Int64", safe=True), "label", "Int64"),
                        (cast(cast(c("a_l"), "Utf8"), "Int64"), "l", "Int64"), (cast(cast(c("a_u"), "Utf8"), "Int64", safe=True), "u", "Int64"),
                        (cast(cast(c("a_u"), "Utf8"), "UInt64"), "uu", "UInt64")])
    elif i == 4:
        e = cast(c("a_m"), "Int64")
        inp = filt(a, binop(e, rnd.choice(["Gt", "LtEq"]), lit("Int64", rnd.choice([100, 0, -2**20]))))
        keys = rnd.choice([[], ["a_g"]])
        node = aggregate(inp, keys, [("sum", (e, "Int64")), ("min", (cast(c("a_n"), "Int32"), "Int32")), ("max", (e, "Int64")), ("count", None)])
    else:
        nc = rnd.choice([300, 4097])
        t["a_n"] = with_nulls(text_numbers("Int64", n, rnd, True, nc + 50), rnd.choice([0.0, 0.02]), r)
        tc = make_table("c", nc, r, rnd)
        jt = "Inner" if seed % 2 == 0 else "Semi"
        below = proj(a, [(cast(c("a_n"), "Int64"), "key", "Int64"), ident, (c("a_s2"), "a_s2", "Utf8")])
        right = keep(scan(table_cols("c")), ["c_id", "c_s"])
        if jt == "Inner":
            node, tables = join("Inner", right, below, [("c_id", "key")]), [tc, t]
        else:
            node, tables = join("Semi", below, right, [("key", "c_id")]), [t, tc]
        if rnd.random() < 0.5:
            node = aggregate(node, ["key"], [("count", None)])
        else:
            node = sort(node, [("key", rnd.random() < 0.5, rnd.random() < 0.5), ("a_id", False, False)])
            ordered = True
    return _finish(node, tables, r, rnd, ordered, "n=%d" % n)


def r_errors_text(seed, i, rnd, r):
    """r_errors for the text casts, exactly ONE failing row at 0, n - 1, a random position or either side of a workgroup (1024) or tile (8192)
    boundary: 0 a Timestamp one millisecond outside the years 0000 to 9999 to Utf8, 1 '2147483648' to Int32, 2 a trailing blank to Int64, 3 '-0'
    to UInt64, 4 '2015-02-29' to Timestamp, 5 a bad text under a filter's predicate"""
    n = size(seed, i, rnd, [1, 65, 700, 1025, 8192, 8193])
    a, t = parse_table(n, r, rnd)
    at = rnd.choice([0, n - 1, rnd.randrange(n)] + ([1023, 1024] if n > 1024 else []) + ([8191, 8192] if n > 8192 else []))
    c = a.c
    if i == 0:
        t["a_t"][at] = rnd.choice([TS_MAX + 1, TS_MIN - 1])
        e, ty = cast(c("a_t"), "Utf8"), "Utf8"
    elif i == 1:
        t["a_n"][at] = "2147483648"
        e, ty = cast(c("a_n"), "Int32"), "Int32"
    elif i == 2:
        t["a_m"][at] = (t["a_m"][at] or "5") + " "
        e, ty = cast(c("a_m"), "Int64"), "Int64"
    elif i == 3:
        t["a_p"][at] = "-0"
        e, ty = cast(c("a_p"), "UInt64"), "UInt64"
    elif i == 4:
        t["a_d"][at] = "2015-02-29"
        e, ty = cast(c("a_d"), "ts"), "ts"
    else:
        t["a_m"][at] = rnd.choice(["", "1e3", "5a", "--5", "9223372036854775808"])
        e, ty = cast(c("a_m"), "Int64"), "Int64"
    if i == 5:
        node = filt(a, binop(e, "Gt", lit("Int64", 0)))
    else:
        node = proj(a, [(c("a_id"), "a_id", "Int64"), (e, "e", ty)])
    return _finish(node, [t], r, rnd, False, "n=%d at=%d" % (n, at))


# ------------------------------------------------------------------ Float64 special values (A-FO1 .. A-FO5 of relops.hpp; tests/float_order_ref.py)
FLOAT_SIZES = [65, 700, 2047, 2049, 4095, 4097, 8193]          # (the window tile is 2048 rows, the sort tile 4096)
FLOAT_LITERALS = [-0.0, 0.0, 5e-324, -5e-324, 1.7976931348623157e308, 1.0]
ORDINARY = [0.25, -1.5, 3.0, 1024.75]
# few distinct values, so that partitions and peer groups hold several rows: both zeros, NaNs of three patterns, a subnormal, -inf, two numbers
FEW_FLOATS = [0x0000000000000000, 0x8000000000000000, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x0000000000000001, 0xFFF0000000000000,
              0x3FF0000000000000, 0x3FD0000000000000]
# either side of what fits Int32, Int64 and UInt64 (tests/test_plan_float_edges.py lists what each gives)
CAST_EDGES = [2147483647.0, 2147483647.9, 2147483648.0, -2147483648.0, -2147483648.9, -2147483649.0, 9223372036854774784.0, 9223372036854775808.0,
              -9223372036854775808.0, -9223372036854777856.0, -0.9, -1.0, 18446744073709549568.0, 18446744073709551616.0]
CMPS = ["Eq", "NotEq", "Lt", "LtEq", "Gt", "GtEq"]


def _not(e):
    return {"physical_expr": "not_expr", "arg": e}


def _flag(cond):
    """a condition as a projected Int32: 1 TRUE, 0 FALSE, NULL for NULL"""
    return case_([(cond, lit("Int32", 1)), (_not(cond), lit("Int32", 0))])


def r_float_special(seed, i, rnd, r):
    """a_f from float_order_ref.SPECIALS, a few quarter-integers and NULLs; a_f2 from the NaN-free part (what MIN / MAX take).  case 0: ORDER BY a_f,
    the four ASC / DESC x nulls first / last pairs over the seeds; case 1: a_f as the second key under a small Int32 key, then a limit -- in odd seeds
    two such limits under a UNION ALL (the ordered NaN payloads cross a copy kernel); case 2: running COUNT, SUM, MIN and MAX with ORDER BY a_f under an
    Int32 partition, the sort WITHOUT the row's number (tied zeros and NaNs arrive interleaved); case 3: PARTITION BY a_f with ROW_NUMBER and one
    aggregate; case 4: a filter of one-pass leaves -- a_f against a literal of FLOAT_LITERALS, against a_f2 and against itself, under AND / OR / NOT
    and IS NULL; case 5: the same comparisons on the general evaluator (a computed right side; as projected flags) and TRY_CAST(a_f AS Int32 /
    Int64 / UInt64) over the pool widened by CAST_EDGES.  Cases 2 and 3 draw a_f from FEW_FLOATS.  CASES_PER_SEED is 6, so no case index is left
    undirected: the mixtures ride on cases 1 and 5 by seed."""
    n = size(seed, i, rnd, FLOAT_SIZES)
    cols = table_cols("a") + [("a_f2", "Float64")]
    t = make_table("a", n, r, rnd, style="dense", card=7, groups=rnd.choice([1, 5]), nulls={"g": 0.0, "v": 0.02, "i": 0.02})
    pool = [fo.from_bits(b) for b in (FEW_FLOATS if i in (2, 3) else fo.SPECIALS)] + (ORDINARY[:1] if i in (2, 3) else ORDINARY) + (CAST_EDGES if i == 5 else [])
    t["a_f"] = pooled(pool, n, r, rnd.choice([0.02, 0.3]))
    t["a_f2"] = pooled([fo.from_bits(b) for b in fo.NAN_FREE] + ORDINARY, n, r, rnd.choice([0.0, 0.02, 0.3]))
    a = scan(cols)
    c = a.c
    desc, nf = [(False, False), (False, True), (True, False), (True, True)][seed % 4]
    ordered = False
    op = lambda k: CMPS[(seed + k) % 6]
    if i == 0:
        node = sort(keep(a, ["a_f", "a_id", "a_v"]), [("a_f", desc, nf), ("a_id", False, False)])
        ordered = True
    elif i == 1:
        src = keep(a, ["a_g", "a_f", "a_id"])
        first = (rnd.random() < 0.5, rnd.random() < 0.5)
        node = limit(sort(src, [("a_g",) + first, ("a_f", desc, nf), ("a_id", False, False)]), rnd.choice([50, 5000]))
        ordered = True
        if seed % 2:
            node = union([node, limit(sort(src, [("a_g",) + first, ("a_f", not desc, nf), ("a_id", True, False)]), 50)])
            ordered = False
    elif i == 2:
        part, order = ["a_g"], ["a_f"]
        srt = sort(a, [("a_g", False, False), ("a_f", False, False)])
        node = window(srt, [("count", None, part, order), ("sum", "a_v", part, order), ("min", "a_f2", part, order), ("max", "a_f2", part, order)])
        node = keep(node, [n_ for n_, _ in node.cols[:4]] + ["a_id", "a_g", "a_f"])
    elif i == 3:
        part, order = ["a_f"], (["a_g"] if seed % 2 else [])
        srt = sort(a, [("a_f", False, False)] + [(o, False, False) for o in order] + [("a_id", False, False)])
        node = window(srt, [("row_number", None, part, []), (("sum", "a_v") if seed < 2 else ("max", "a_f2")) + (part, order)])
        node = keep(node, [n_ for n_, _ in node.cols[:2]] + ["a_id", "a_f"] + order)
    elif i == 4:
        l1 = binop(c("a_f"), op(4), lit("Float64", FLOAT_LITERALS[seed % 6]))
        l2 = binop(c("a_f"), op(1), c("a_f2"))
        l3 = {"physical_expr": rnd.choice(["is_null_expr", "is_not_null_expr"]), "arg": c("a_f2")}
        l4 = binop(c("a_f"), ["Eq", "NotEq", "LtEq", "Lt"][seed % 4], c("a_f"))       # TRUE for no NaN (=, <=), for every NaN (<>), for nothing (<)
        l5 = binop(lit("Float64", rnd.choice(FLOAT_LITERALS)), op(2), c("a_f"))       # the literal on the left
        pred = binop(binop(l1, "And", _not(l2)), "Or", binop(l4, "And", binop(l5, "Or", l3)))
        node = keep(filt(a, pred), ["a_id", "a_f", "a_f2"])
    else:
        right = binop(c("a_f2"), "Plus", lit("Float64", 0.0))                          # a computed right side: no one-pass leaf, the general evaluator
        outs = [(c("a_id"), "a_id", "Int64"), (c("a_f"), "a_f", "Float64")]
        outs += [(cast(c("a_f"), ty, safe=True), "to_" + ty, ty) for ty in ("Int32", "Int64", "UInt64")]
        outs += [(_flag(binop(c("a_f"), op(k), c("a_f2") if k % 2 else lit("Float64", FLOAT_LITERALS[(seed + k) % 6]))), "is%d" % k, "Int32") for k in range(3)]
        outs.append((_flag(binop(c("a_f"), "Eq", c("a_f"))), "self", "Int32"))
        inp = a
        if seed % 2:
            inp = filt(a, binop(binop(c("a_f"), op(3), right), "Or", _not(binop(c("a_f"), op(5), right))))
        node = proj(inp, outs)
    return Case(node.plan, [t], [cuts(n, r, rnd)], ordered, "n=%d %s nulls_first=%s" % (n, "DESC" if desc else "ASC", nf))


ERROR_STRATA = ("errors", "errors_text")

_RECIPES = {"filter_project": r_filter_project, "text": r_text, "group_narrow": r_group_narrow, "group_composite": r_group_composite, "group_wide": r_group_wide,
            "distinct_count": r_distinct_count, "global_agg": r_global_agg, "join_inner": r_join_inner, "join_semi_anti": r_join_semi_anti,
            "sort_limit": r_sort_limit, "window": r_window, "cross": r_cross, "mixed": r_mixed, "errors": r_errors,
            "union": r_union, "cast_text": r_cast_text, "parse_text": r_parse_text, "errors_text": r_errors_text, "float_special": r_float_special}


def case(stratum, seed, i):
    rnd, r = _rngs(stratum, seed, i)
    return _RECIPES[stratum](seed, i, rnd, r)


def generic_only(stratum, seed, i):
    """roughly half of the cases run with the fused NEXMark pipelines switched off (flockgpu_plan_create_ex's flag)"""
    return (STRATA.index(stratum) + seed + i) % 2 == 0
