"""A plan-JSON interpreter on the CPU: run_plan(plan, tables) walks a serialised plan of the dialect the README claims and evaluates every node with plain
Python values -- int, float, str, None for NULL -- row at a time.  It is the reference of tests/test_plan_differential.py.

What it is made of: oracle.generic_ops (the typed expression rules: wrap-around, checked casts, the failing divisions; the stable multi-key sort; the
inner join's build / probe; limit), scalar_fn_ref (every scalar function), text_slice_ref (the slice functions), test_plan_like.reference_like (LIKE),
wide_group_ref.finish (COUNT / SUM / MIN / MAX / AVG of one group: SUM wraps in 64 bits, AVG is one division), count_distinct_ref (distinct counts),
semi_anti_ref (Semi / Anti), cross_join_ref (the pair order), union_ref (UNION ALL), cast_text_ref (integers and timestamps as text), parse_text_ref (text as
integers and timestamps), float_order_ref (how Float64 keys order and tie: A-FO1, A-FO2, A-FO4 of relops.hpp; comparisons stay Python's IEEE).  The tree walk, the typing of expressions that carry a function, and the window frame are
restated here; test_plan_differential.py pins the result to the reference's transcribed vectors and to every one of those modules on its own table.

Where the parts disagree: generic_ops.hash_aggregate_exec adds SUM without wrapping and AVG as a running Float64 sum, wide_group_ref wraps SUM in 64 bits
and divides the wrapped sum once.  The README's rule is the second (`groupwide.hpp`), and the two agree wherever no sum leaves 64 bits and every prefix
sum is exact in Float64; the interpreter takes wide_group_ref's.

`quirks` switches single rules to a plausible WRONG neighbour (QUIRKS below), so that a test can prove that a corpus tells the two apart.

A relation is (names, types, columns); a type is 'Int32' | 'Int64' | 'UInt64' | 'Float64' | 'Utf8' | 'Boolean' | {"Timestamp": ["Millisecond", None]}."""
import datetime as _dtm
import functools
import re

import cast_text_ref as ctref
import count_distinct_ref as dref
import cross_join_ref as xref
import float_order_ref as fo
import parse_text_ref as ptref
import scalar_fn_ref as sref
import semi_anti_ref as saref
import text_slice_ref as tsl
import union_ref as uref
import wide_group_ref as wref
from oracle import generic_ops as g
from oracle.generic_ops import ExprError

TS = sref.TS

# quirk -> the stratum of tests/plan_corpus.py whose cases must tell it from the true rule
QUIRKS = {
    "join_null_equals_null": "join_inner",                 # a NULL join key matches a NULL join key
    "anti_drops_null_keys": "join_semi_anti",              # Anti drops a NULL-keyed left row as Semi does
    "semi_row_per_partner": "join_semi_anti",              # Semi returns a left row once per partner
    "count_col_counts_nulls": "group_narrow",              # COUNT(col) counts NULLs
    "sum_of_nothing_is_zero": "global_agg",                # SUM over no valid value is 0, not NULL
    "avg_int_truncates": "group_narrow",                   # AVG of integers is an integer division
    "div_floors": "filter_project",                        # integer / floors instead of truncating
    "mod_sign_of_divisor": "filter_project",               # % takes the divisor's sign
    "int32_arith_does_not_wrap": "filter_project",         # Int32 arithmetic is carried out in 64 bits
    "or_null_true_is_null": "filter_project",              # NULL OR TRUE is NULL
    "filter_keeps_null_predicate": "filter_project",       # a filter keeps the rows whose predicate is NULL
    "case_null_condition_is_true": "text",                 # a NULL WHEN condition selects its branch
    "group_drops_null_keys": "group_composite",            # rows with a NULL group key form no group
    "minmax_u64_as_signed": "group_wide",                  # MIN / MAX of UInt64 compare as Int64
    "nulls_first_ignored": "sort_limit",                   # NULLs always last
    "desc_moves_nulls": "sort_limit",                      # DESC flips where the NULLs go
    "sort_ties_reversed": "sort_limit",                    # every key pass leaves its ties reversed
    "utf8_prefix_sorts_last": "sort_limit",                # a proper prefix sorts after the longer value
    "like_underscore_is_one_byte": "filter_project",       # `_` steps over one byte
    "left_counts_bytes": "text",                           # left(s, n) counts bytes
    "window_frame_excludes_peers": "window",               # the frame ends at the row itself (ROWS, not RANGE)
    "distinct_counts_null": "distinct_count",              # NULL is one of the distinct values
    "date_trunc_towards_zero_before_1970": "filter_project",
    "week_starts_sunday": "filter_project",
    "cross_pair_order_swapped": "cross",                   # pair (i, j) at output row j * L + i
    "union_inputs_reversed": "union",                      # the last input's rows come first
    "union_is_distinct": "union",                          # the union drops duplicate rows (UNION, not UNION ALL)
    "ts_text_always_prints_millis": "cast_text",           # a whole second prints its `.000`
    "ts_text_truncates_towards_zero_before_1970": "cast_text",   # -1 prints as 1970-01-01 00:00:00.001
    "uint64_text_as_signed": "cast_text",                  # a UInt64 at or above 2^63 prints as the Int64 of its bits
    "parse_refuses_leading_plus": "parse_text",            # `+5` does not parse (pyarrow's rule)
    "parse_trims_blanks": "parse_text",                    # blanks around a value are skipped
    "parse_minus_zero_is_uint64_zero": "parse_text",       # `-0` is the UInt64 0
    "try_cast_bad_text_is_zero": "parse_text",             # try_cast_expr of a text that does not parse gives 0, not NULL
    "nan_ordered_by_sign": "float_special",                # a NaN with the sign bit set sorts before -inf (the order of the bit patterns)
    "zeros_ordered_by_sign": "float_special",              # -0.0 sorts before +0.0, whatever the input order
    "float_peers_by_bits": "float_special",                # window partitions and peer groups compare Float64 keys by their bit patterns
    "nan_equals_itself": "float_special",                  # f = f is TRUE for a NaN
    "subnormals_are_zero": "float_special",                # a subnormal compares as 0
    "float_cast_saturates": "float_special",               # a TRY_CAST of a Float64 that does not fit clamps (NaN: 0) instead of giving NULL
}

_NEUTRAL = ("coalesce_batches_exec", "repartition_exec", "coalesce_partitions_exec", "merge_exec")
_ARITH = ("Plus", "Minus", "Multiply", "Divide", "Modulo")
_CMP = ("Eq", "NotEq", "Lt", "LtEq", "Gt", "GtEq")
_INT = g._INT_RANGE
_UNIT_MS = {"second": 1000, "minute": 60_000, "hour": 3_600_000, "day": 86_400_000}
_NUM_AS_TEXT = ("Int32", "Int64", "UInt64")              # and Timestamp(ms): the operands of a cast to Utf8
_MINUS_ZERO = re.compile(r"-0+")


class Rel:
    __slots__ = ("names", "types", "cols")

    def __init__(self, names, types, cols):
        self.names, self.types, self.cols = list(names), list(types), [list(c) for c in cols]

    @property
    def n(self):
        return len(self.cols[0]) if self.cols else 0

    def rows(self):
        return list(zip(*self.cols)) if self.cols else []

    def tmap(self):
        return dict(zip(self.names, self.types))

    def dicts(self):
        return [dict(zip(self.names, r)) for r in self.rows()]

    def take(self, idx):
        return Rel(self.names, self.types, [[c[i] for i in idx] for c in self.cols])


def _is_ts(t):
    return isinstance(t, dict) and "Timestamp" in t


def _fn_name(e):
    name = (e.get("name") or e.get("fun")).lower()
    return sref.ALIASES.get(name, name)


def full_type(e, types):
    """The type of an expression as a schema carries it (Timestamp stays Timestamp); None for a literal that takes the type of what it meets."""
    t = e["physical_expr"]
    if t == "column":
        return types[e["name"]]
    if t == "literal":
        v = e["value"]
        kind = next(iter(v)) if isinstance(v, dict) and v else None
        val = next(iter(v.values())) if isinstance(v, dict) and v else v
        if kind == "Utf8" or isinstance(val, str):
            return "Utf8"
        if val is None:
            return None
        if kind == "Boolean" or isinstance(val, bool):
            return "Boolean"
        if kind in ("Float64", "Float32") or isinstance(val, float):
            return "Float64"
        return kind if kind in _INT else None
    if t in ("cast_expr", "try_cast_expr"):
        return e["cast_type"]
    if t == "negative_expr":
        return full_type(e.get("arg", e.get("expr")), types)
    if t in ("not_expr", "is_null_expr", "is_not_null_expr", "in_list_expr"):
        return "Boolean"
    if t == "binary_expr":
        if e["op"] not in _ARITH:
            return "Boolean"
        a = full_type(e["left"], types)
        return a if a is not None else full_type(e["right"], types)
    if t == "case_expr":
        for _, th in e["when_then_expr"]:
            ty = full_type(th, types)
            if ty is not None:
                return ty
        return full_type(e["else_expr"], types) if e.get("else_expr") else None
    if t == "scalar_function_expr":
        name = _fn_name(e)
        if name in tsl.SLICE_FNS:
            return "Utf8"
        if name in sref.MATH or name in ("date_trunc", "date_part", "now", "octet_length", "char_length"):
            return sref.result_type(name)
        raise NotImplementedError("scalar function " + name)
    raise NotImplementedError("physical_expr " + str(t))


def _st(e, types):
    return g._type_name(full_type(e, types))


def _prefix_cmp(a, b):
    """the WRONG bytewise order of utf8_prefix_sorts_last: a proper prefix after the longer value"""
    x, y = a.encode(), b.encode()
    if x == y:
        return 0
    if y.startswith(x):
        return 1
    if x.startswith(y):
        return -1
    return -1 if x < y else 1


def _is_f64(ty):
    return ty == "Float64"


def _flush(v):
    """subnormals_are_zero: a subnormal operand as the zero of its sign"""
    return v * 0.0 if isinstance(v, float) and v == v and 0.0 < abs(v) < 2.2250738585072014e-308 else v


class _Interp:
    def __init__(self, tables, quirks):
        self.tables, self.q = tables, frozenset(quirks)
        unknown = self.q - set(QUIRKS)
        if unknown:
            raise ValueError("unknown quirks: %s" % sorted(unknown))
        self.leaves = {}

    def assign(self, plan):
        schemas = leaf_schemas(plan)
        if len(schemas) != len(self.tables):
            raise ValueError("%d leaves of different schemas, %d tables" % (len(schemas), len(self.tables)))
        self.leaves = {tuple(f["name"] for f in fields): t for fields, t in zip(schemas, self.tables)}
        return self

    # ------------------------------------------------------------------ expressions
    def like(self, value, pattern):
        if "like_underscore_is_one_byte" in self.q:
            rx = b"".join(b".*" if c == "%" else b"." if c == "_" else re.escape(c.encode()) for c in pattern)
            return re.fullmatch(rx, value.encode(), re.S) is not None
        from test_plan_like import reference_like
        return reference_like(value.encode(), pattern)

    def call(self, name, args):
        if name in tsl.SLICE_FNS:
            if args[0] is None:
                return None
            if name == "left" and "left_counts_bytes" in self.q:
                n = args[1]
                b = args[0].encode()
                return (b[:n] if n >= 0 else b[:max(len(b) + n, 0)]).decode("utf-8", "replace")
            return tsl._FN[name](*args)
        if name == "now":
            raise NotImplementedError("now() has no value a test can expect")
        if any(a is None for a in args):
            return None
        if name == "date_trunc":
            unit, ms = args[0].lower(), args[1]
            if "date_trunc_towards_zero_before_1970" in self.q and ms < 0 and unit in _UNIT_MS:
                return -(-ms // _UNIT_MS[unit] * _UNIT_MS[unit])
            if "week_starts_sunday" in self.q and unit == "week":
                d = sref._when(ms // sref.MS_DAY * sref.MS_DAY)
                return sref._ms(d - _dtm.timedelta(days=(d.weekday() + 1) % 7))
        return sref.call(name, args)

    def num_text(self, v, src, safe):
        """CAST(v AS Utf8) of one non-NULL integer or Timestamp(ms): cast_text_ref.int_text / ts_text"""
        q = self.q
        if not _is_ts(src):
            if src == "UInt64" and v >= 2**63 and "uint64_text_as_signed" in q:
                v -= 2**64
            return ctref.int_text([v])[0]
        try:
            if "ts_text_truncates_towards_zero_before_1970" in q and v < 0 and v % 1000:
                whole = ctref.ts_text([(v // 1000 + 1) * 1000], safe)[0]
                return whole if whole is None else "%s.%03d" % (whole, -v % 1000)
            text = ctref.ts_text([v], safe)[0]
        except ctref.CastRangeError as err:
            raise ExprError(str(err))
        if text is not None and "ts_text_always_prints_millis" in q and v % 1000 == 0:
            text += ".000"
        return text

    def text_num(self, s, target, safe):
        """CAST(s AS target) of one non-NULL text: parse_text_ref.parse_one"""
        q = self.q
        if "parse_trims_blanks" in q:
            s = s.strip(" ")
        v = ptref.parse_one(s, target)
        if "parse_refuses_leading_plus" in q and s.startswith("+"):
            v = None
        if "parse_minus_zero_is_uint64_zero" in q and target == "UInt64" and _MINUS_ZERO.fullmatch(s):
            v = 0
        if v is None:
            if not safe:
                raise ExprError("%r is no %s" % (s, target))
            if "try_cast_bad_text_is_zero" in q:
                return 0
        return v

    def ev(self, e, row, types, want=None):
        """generic_ops.eval_typed, with scalar functions, LIKE, text values and the quirks.  Every branch of eval_typed is kept in its words."""
        q = self.q
        t = e["physical_expr"]
        if t == "column":
            return row[e["name"]]
        if t == "literal":
            v = g.eval_physical_expr(e, row) if not (isinstance(e["value"], dict) and not e["value"]) else None
            if isinstance(v, int) and not isinstance(v, bool) and (_st(e, types) or want) == "Float64":
                return float(v)
            return v
        if t in ("cast_expr", "try_cast_expr"):
            v = self.ev(e["expr"], row, types)
            ty = g._type_name(e["cast_type"])
            src = full_type(e["expr"], types)
            literal = e["expr"]["physical_expr"] == "literal"
            if ty == "Utf8":
                if src == "Utf8":
                    return v
                if literal or not (src == TS or src in _NUM_AS_TEXT):
                    raise NotImplementedError("a cast of %s to Utf8" % ("a literal" if literal else src))
                return None if v is None else self.num_text(v, src, t == "try_cast_expr")
            if src == "Utf8":
                target = "Timestamp" if e["cast_type"] == TS else e["cast_type"]
                if literal or target not in ptref.TARGETS:
                    raise NotImplementedError("a cast of %s to %s" % ("a text literal" if literal else "text", e["cast_type"]))
                return None if v is None else self.text_num(v, target, t == "try_cast_expr")
            if ty not in _INT and ty != "Float64":
                raise NotImplementedError("cast to " + str(ty))
            if v is not None and t == "try_cast_expr" and isinstance(v, float) and ty in _INT and "float_cast_saturates" in q:
                lo, hi = _INT[ty]
                return 0 if v != v else lo if v < lo else hi if v > hi else int(v)
            return None if v is None else g._cast(v, ty, t == "try_cast_expr")
        if t == "negative_expr":
            a = e.get("arg", e.get("expr"))
            v = self.ev(a, row, types, want)
            ty = _st(a, types) or want
            return None if v is None else (-v if (ty == "Int32" and "int32_arith_does_not_wrap" in q) else g._wrap(-v, ty))
        if t == "not_expr":
            v = self.ev(e.get("arg", e.get("expr")), row, types, "Boolean")
            return None if v is None else (not v)
        if t == "is_null_expr":
            return self.ev(e.get("arg", e.get("expr")), row, types) is None
        if t == "is_not_null_expr":
            return self.ev(e.get("arg", e.get("expr")), row, types) is not None
        if t == "in_list_expr":
            ty = _st(e["expr"], types)
            v = self.ev(e["expr"], row, types)
            if v is None:
                return None
            hit = any(v == self.ev(x, row, types, ty) for x in e["list"])
            return (not hit) if e.get("negated") else hit
        if t == "case_expr":
            ty = _st(e, types) or want
            out = self.ev(e["else_expr"], row, types, ty) if e.get("else_expr") else None
            for w, th in reversed(e["when_then_expr"]):
                then = self.ev(th, row, types, ty)
                if e.get("expr"):
                    tb = _st(e["expr"], types) or _st(w, types)
                    a, b = self.ev(e["expr"], row, types, tb), self.ev(w, row, types, tb)
                    cond = None if a is None or b is None else a == b
                else:
                    cond = self.ev(w, row, types, "Boolean")
                if cond is True or (cond is None and "case_null_condition_is_true" in q):
                    out = then
            return out
        if t == "scalar_function_expr":
            name = _fn_name(e)
            full_type(e, types)
            args = []
            for k, a in enumerate(e.get("args", [])):
                args.append(self.ev(a, row, types))
            if name in ("date_trunc", "date_part"):
                if not _is_ts(full_type(e["args"][1], types)):
                    raise NotImplementedError(name + " of something that is not a Timestamp")
            elif name in sref.MATH and _st(e["args"][0], types) != "Float64":
                raise NotImplementedError(name + " of an integer")
            return self.call(name, args)
        if t == "binary_expr":
            op = e["op"]
            if op in ("And", "Or"):
                a, b = self.ev(e["left"], row, types, "Boolean"), self.ev(e["right"], row, types, "Boolean")
                if op == "And":
                    return False if (a is False or b is False) else (None if (a is None or b is None) else True)
                if "or_null_true_is_null" in q and (a is None or b is None):
                    return None
                return True if (a is True or b is True) else (None if (a is None or b is None) else False)
            if op in ("Like", "NotLike"):
                a, b = self.ev(e["left"], row, types), self.ev(e["right"], row, types)
                if a is None or b is None:
                    return None
                return self.like(a, b) != (op == "NotLike")
            if op not in _ARITH and op not in _CMP:
                raise NotImplementedError("binary operator " + op)
            ty = _st(e["left"], types) or _st(e["right"], types) or (want if op in _ARITH else None)
            a, b = self.ev(e["left"], row, types, ty), self.ev(e["right"], row, types, ty)
            if a is None or b is None:
                return None
            if op in _CMP:
                if isinstance(a, str) and "utf8_prefix_sorts_last" in q and op not in ("Eq", "NotEq"):
                    c = _prefix_cmp(a, b)
                    return {"Lt": c < 0, "LtEq": c <= 0, "Gt": c > 0, "GtEq": c >= 0}[op]
                if "subnormals_are_zero" in q:
                    a, b = _flush(a), _flush(b)
                if "nan_equals_itself" in q and isinstance(a, float) and isinstance(b, float) and a != a and b != b:
                    return op in ("Eq", "LtEq", "GtEq")
                return {"Eq": a == b, "NotEq": a != b, "Lt": a < b, "LtEq": a <= b, "Gt": a > b, "GtEq": a >= b}[op]
            if ty == "Float64" or isinstance(a, float) or isinstance(b, float):
                import numpy as np
                x, y = np.float64(a), np.float64(b)
                if op in ("Divide", "Modulo") and y == 0:
                    raise ExprError("division by zero")
                with np.errstate(all="ignore"):
                    return float({"Plus": x + y, "Minus": x - y, "Multiply": x * y, "Divide": x / y, "Modulo": np.fmod(x, y)}[op])
            wrap = (lambda v, _t: v) if (ty == "Int32" and "int32_arith_does_not_wrap" in q) else g._wrap
            if op in ("Divide", "Modulo"):
                if b == 0:
                    raise ExprError("division by zero")
                if b == -1 and ty in _INT and ty != "UInt64" and a == _INT[ty][0]:
                    raise ExprError("INT_MIN / -1 overflows")
                if op == "Modulo":
                    return wrap(a % b if "mod_sign_of_divisor" in q else g._trunc_mod(a, b), ty)
                if "div_floors" in q:
                    return wrap(a // b, ty)
                k = abs(a) // abs(b)
                return wrap(k if (a >= 0) == (b >= 0) else -k, ty)
            return wrap({"Plus": a + b, "Minus": a - b, "Multiply": a * b}[op], ty)
        raise NotImplementedError("physical_expr " + str(t))

    def column(self, e, rel, want=None):
        """(type, values) of expression `e` over every row of `rel`"""
        types = rel.tmap()
        if e["physical_expr"] == "column" and e["name"] not in types:
            if "index" not in e:
                raise KeyError(e["name"])
            return rel.types[e["index"]], rel.cols[e["index"]]
        ty = full_type(e, types)
        if e["physical_expr"] == "column":
            return ty, rel.cols[rel.names.index(e["name"])]
        w = want or g._type_name(ty)
        return ty, [self.ev(e, r, types, w) for r in rel.dicts()]

    # ------------------------------------------------------------------ nodes
    def run(self, node):
        kind = node.get("execution_plan")
        f = getattr(self, "n_" + str(kind), None)
        if kind in _NEUTRAL:
            return self.run(node["input"])
        if f is None:
            raise NotImplementedError("execution_plan " + str(kind))
        return f(node)

    def n_memory_exec(self, node):
        fields = node["schema"]["fields"]
        t = self.leaves[tuple(f["name"] for f in fields)]
        proj = node.get("projection")
        if proj is not None:
            fields = [fields[i] for i in proj]
        for f in fields:
            if g._type_name(f["data_type"]) not in ("Int32", "Int64", "UInt64", "Float64", "Utf8"):
                raise NotImplementedError("column type " + str(f["data_type"]))
        return Rel([f["name"] for f in fields], [f["data_type"] for f in fields], [t[f["name"]] for f in fields])

    def n_filter_exec(self, node):
        rel = self.run(node["input"])
        types = rel.tmap()
        keep = []
        for i, r in enumerate(rel.dicts()):
            v = self.ev(node["predicate"], r, types, "Boolean")
            if v is True or (v is None and "filter_keeps_null_predicate" in self.q):
                keep.append(i)
        return rel.take(keep)

    def n_projection_exec(self, node):
        rel = self.run(node["input"])
        out = [self.column(e, rel) for e, _ in node["expr"]]
        types = [ty for ty, _ in out]
        if any(ty is None or ty == "Boolean" for ty in types):
            raise NotImplementedError("a projected column without a column type")
        return Rel([n for _, n in node["expr"]], types, [c for _, c in out])

    def n_global_limit_exec(self, node):
        rel = self.run(node["input"])
        return rel.take(range(min(node["limit"], rel.n)))

    def float_key(self, x):
        """float_order_ref.key (A-FO1), or one of its wrong neighbours"""
        k = fo.key(x)
        if "nan_ordered_by_sign" in self.q and k[0] == 1 and fo.bits(x) >> 63:
            k = (-1, 0.0)
        if "zeros_ordered_by_sign" in self.q and k == (0, 0.0):
            k = (0, 0.0, -1 if fo.bits(x) >> 63 else 0)
        return k

    def group_key(self, ty, v):
        """what the window's partition / peer tests and ROW_NUMBER's runs compare (A-FO2): float_order_ref.same for Float64"""
        if v is None or not _is_f64(ty) or not isinstance(v, float):
            return v
        return ("bits", fo.bits(v)) if "float_peers_by_bits" in self.q else fo.key(v)

    def sort_index(self, rel, specs):
        """generic_ops.sort_exec's passes (last key first, each stable) over computed key columns"""
        q = self.q
        idx = list(range(rel.n))
        keys = [(self.column(s["expr"], rel), s["options"]["descending"], s["options"]["nulls_first"]) for s in specs]
        for (ty, col), desc, nulls_first in reversed(keys):
            if "sort_ties_reversed" in q:
                idx.reverse()
            if "nulls_first_ignored" in q:
                nulls_first = False
            if "desc_moves_nulls" in q and desc:
                nulls_first = not nulls_first
            vals = [i for i in idx if col[i] is not None]
            nulls = [i for i in idx if col[i] is None]
            if ty == "Utf8" and "utf8_prefix_sorts_last" in q:
                vals.sort(key=functools.cmp_to_key(lambda i, j: _prefix_cmp(col[i], col[j])), reverse=desc)
            elif _is_f64(ty):
                vals.sort(key=lambda i: self.float_key(col[i]), reverse=desc)
            else:
                vals.sort(key=lambda i: col[i], reverse=desc)
            idx = nulls + vals if nulls_first else vals + nulls
        return idx

    def n_sort_exec(self, node):
        rel = self.run(node["input"])
        return rel.take(self.sort_index(rel, node["expr"]))

    def n_cross_join_exec(self, node):
        l, r = self.run(node["left"]), self.run(node["right"])
        if "cross_pair_order_swapped" in self.q:
            rows = [a + b for b in r.rows() for a in l.rows()]
        else:
            rows = xref.cross_rows(l.rows(), r.rows())
        cols = list(zip(*rows)) if rows else [()] * (len(l.names) + len(r.names))
        return Rel(l.names + r.names, l.types + r.types, cols)

    def n_union_exec(self, node):
        rels = [self.run(x) for x in node["inputs"]]
        if not rels:
            raise NotImplementedError("a union_exec without inputs")
        for k, r in enumerate(rels[1:], 1):
            if r.types != rels[0].types:
                raise NotImplementedError("union_exec: input %d gives %s, input 0 gives %s" % (k, r.types, rels[0].types))
        if "union_inputs_reversed" in self.q:
            rels = rels[::-1]
        rows = uref.union_rows([r.rows() for r in rels])
        if "union_is_distinct" in self.q:
            rows = list(dict.fromkeys(rows))
        first = rels[-1 if "union_inputs_reversed" in self.q else 0]
        return Rel(first.names, first.types, list(zip(*rows)) if rows else [()] * len(first.names))

    def n_hash_join_exec(self, node):
        jt = node.get("join_type")
        if jt not in ("Inner", "Semi", "Anti"):
            raise NotImplementedError("join_type " + str(jt))
        l, r = self.run(node["left"]), self.run(node["right"])
        on = [((a if isinstance(a, str) else a["name"]), (b if isinstance(b, str) else b["name"])) for a, b in node["on"]]
        lt, rt = l.tmap(), r.tmap()
        for a, b in on:
            ta, tb = g._type_name(lt[a]), g._type_name(rt[b])
            if "Float64" in (ta, tb) or (ta == "Utf8") != (tb == "Utf8"):
                raise NotImplementedError("join key types %s = %s" % (ta, tb))
        lk = [tuple(l.cols[l.names.index(a)][i] for a, _ in on) for i in range(l.n)]
        rk = [tuple(r.cols[r.names.index(b)][j] for _, b in on) for j in range(r.n)]
        if jt == "Inner":   # generic_ops.hash_join_inner: build LEFT, probe RIGHT in row order
            null_ok = "join_null_equals_null" in self.q
            build = {}
            for i, k in enumerate(lk):
                if null_ok or all(v is not None for v in k):
                    build.setdefault(k, []).append(i)
            pairs = [(i, j) for j, k in enumerate(rk) for i in build.get(k, ())]
            return Rel(l.names + r.names, l.types + r.types,
                       [[c[i] for i, _ in pairs] for c in l.cols] + [[c[j] for _, j in pairs] for c in r.cols])
        anti = jt == "Anti"
        keep = saref.semi_anti_rows({str(k): [t[k] for t in lk] for k in range(len(on))}, {str(k): [t[k] for t in rk] for k in range(len(on))},
                                    [(str(k), str(k)) for k in range(len(on))], anti)
        if not on or (not lk and not rk):
            keep = list(range(l.n)) if anti else []
        if anti and "anti_drops_null_keys" in self.q:
            keep = [i for i in keep if all(v is not None for v in lk[i])]
        if not anti and "semi_row_per_partner" in self.q:
            count = {}
            for k in rk:
                count[k] = count.get(k, 0) + 1
            keep = [i for i in keep for _ in range(count[lk[i]])]
        return l.take(keep)

    # -- aggregates
    def finish(self, fn, vals, n_rows, ty):
        """one aggregate of one group: wide_group_ref.finish / count_distinct_ref._finish"""
        q = self.q
        a = g._type_name(ty) if ty is not None else None
        if fn == "dc":
            if "distinct_counts_null" in q:
                return len(set(vals))
            return dref._finish("dc", vals, n_rows)
        if fn == "count":
            if vals is not None and "count_col_counts_nulls" in q:
                return len(vals)
            return wref.finish("count", vals, n_rows)
        live = [v for v in vals if v is not None]
        if fn == "sum" and not live and "sum_of_nothing_is_zero" in q:
            return 0
        if fn == "avg" and live and "avg_int_truncates" in q and a != "Float64":
            s = wref.wrapped_sum(live)
            k = abs(s) // len(live)
            return float(k if s >= 0 else -k)
        if fn in ("min", "max") and a == "UInt64" and live and "minmax_u64_as_signed" in q:
            return (min if fn == "min" else max)(live, key=lambda v: v - 2**64 if v >= 2**63 else v)
        if fn in ("sum", "avg") and a == "Float64":
            raise NotImplementedError("SUM / AVG of Float64")
        if fn in ("sum", "avg", "min", "max") and a not in ("Int32", "Int64", "UInt64", "Float64"):
            raise NotImplementedError("%s of %s" % (fn, a))
        if fn in ("min", "max") and a == "Float64":            # A-FO4: the order of the order keys (wide_group_ref's rule where no NaN goes in)
            return (min if fn == "min" else max)(live, key=fo.total_key) if live else None
        return wref.finish(fn, vals, n_rows, a == "UInt64")

    @staticmethod
    def result_type(fn, ty):
        if fn in ("count", "dc"):
            return "UInt64"
        if fn == "avg":
            return "Float64"
        if fn == "sum":
            return "UInt64" if g._type_name(ty) == "UInt64" else "Int64"
        return ty

    def entries(self, aggr_expr, rel):
        """-> [(fn, name, argument type, argument values or None for COUNT(*))]"""
        out = []
        for a in aggr_expr:
            fn = a["aggregate_expr"].lower()
            if fn in ("distinct_count", "count_distinct"):
                fn = "dc"
            if fn not in ("count", "sum", "min", "max", "avg", "dc"):
                raise NotImplementedError("aggregate_expr " + fn)
            e = a["exprs"][0] if "exprs" in a else a["expr"]
            if e["physical_expr"] == "literal":
                if fn != "count":
                    raise NotImplementedError(fn + " of a literal")
                out.append((fn, a["name"], None, None))
                continue
            ty, vals = self.column(e, rel)
            if fn == "dc" and g._type_name(ty) == "Float64":
                raise NotImplementedError("COUNT(DISTINCT) of Float64")
            out.append((fn, a["name"], ty, vals))
        return out

    def groups(self, rel, group_expr):
        """-> (key names, key types, {key tuple: row numbers} in order of first appearance); no keys: ONE group, over no rows too"""
        kcols = [self.column(e, rel) for e, _ in group_expr]
        for ty, _ in kcols:
            if g._type_name(ty) not in ("Int32", "Int64", "UInt64", "Utf8"):
                raise NotImplementedError("GROUP BY key of type " + str(ty))
        groups = {}
        if not group_expr:
            groups[()] = list(range(rel.n))
        else:
            for i in range(rel.n):
                k = tuple(c[i] for _, c in kcols)
                if "group_drops_null_keys" in self.q and any(v is None for v in k):
                    continue
                groups.setdefault(k, []).append(i)
        return [n for _, n in group_expr], [ty for ty, _ in kcols], groups

    def n_hash_aggregate_exec(self, node):
        mode = node.get("mode")
        if mode not in ("Partial", "Final", "FinalPartitioned"):
            raise NotImplementedError("aggregate mode " + str(mode))
        below = node["input"]
        while below.get("execution_plan") in _NEUTRAL:
            below = below["input"]
        partial_below = below.get("execution_plan") == "hash_aggregate_exec" and below.get("mode") == "Partial"
        if mode != "Partial" and not partial_below:
            return self.final_over_states(node)
        src = below if (mode != "Partial" and partial_below) else node      # Final over the Partial of the same plan: ONE aggregation
        rel = self.run(src["input"])
        knames, ktypes, groups = self.groups(rel, src["group_expr"])
        ents = self.entries(node["aggr_expr"], rel)
        names, types, cols = list(knames), list(ktypes), [[k[j] for k in groups] for j in range(len(knames))]
        for fn, name, ty, vals in ents:
            per = [self.finish(fn, None if vals is None else [vals[i] for i in rows], len(rows), ty) for rows in groups.values()]
            if mode != "Partial":
                names.append(name), types.append(self.result_type(fn, ty)), cols.append(per)
            elif fn == "dc":
                raise NotImplementedError("the Partial state of a distinct count (a List column)")
            elif fn == "avg":
                cnt = [self.finish("count", [vals[i] for i in rows], len(rows), ty) for rows in groups.values()]
                sums = [self.finish("sum", [vals[i] for i in rows], len(rows), ty) for rows in groups.values()]
                names += [name + "[count]", name + "[sum]"]
                types += ["UInt64", "Float64"]
                cols += [cnt, [0.0 if s is None else float(s) for s in sums]]
            else:
                names.append("%s[%s]" % (name, fn)), types.append(self.result_type(fn, ty)), cols.append(per)
        return Rel(names, types, cols)

    def final_over_states(self, node):
        """Final / FinalPartitioned over state columns that come from a leaf: keys first, then every aggregate's states by position"""
        rel = self.run(node["input"])
        nk = len(node["group_expr"])
        knames, ktypes, groups = self.groups(rel, [[{"physical_expr": "column", "name": rel.names[i], "index": i}, n]
                                                   for i, (_, n) in enumerate(node["group_expr"])])
        names, types, cols = list(knames), list(ktypes), [[k[j] for k in groups] for j in range(nk)]
        at = nk
        for a in node["aggr_expr"]:
            fn = a["aggregate_expr"].lower()
            if fn not in ("count", "sum", "min", "max", "avg"):
                raise NotImplementedError("a Final of %s over a leaf" % fn)
            st, sty = rel.cols[at], rel.types[at]
            if fn == "avg":
                sums = rel.cols[at + 1]
                per = []
                for rows in groups.values():
                    c = sum(st[i] for i in rows if st[i] is not None)
                    per.append(None if c == 0 else sum(sums[i] for i in rows if sums[i] is not None) / float(c))
                at += 2
                names.append(a["name"]), types.append("Float64"), cols.append(per)
                continue
            how = "sum" if fn == "count" else fn
            per = [self.finish(how, [st[i] for i in rows], len(rows), sty) for rows in groups.values()]
            if fn == "count":
                per = [0 if v is None else v for v in per]
            at += 1
            names.append(a["name"]), types.append(sty), cols.append(per)
        return Rel(names, types, cols)

    # -- window
    def n_window_agg_exec(self, node):
        rel = self.run(node["input"])
        n = rel.n
        names, types, cols = [], [], []
        for w in node["window_expr"]:
            if w.get("window_frame") is not None:
                raise NotImplementedError("an explicit window frame")
            part = [self.column(e, rel) for e in w.get("partition_by", [])]
            order = [self.column(s["expr"], rel) for s in w.get("order_by", [])]
            pkey = [tuple(self.group_key(ty, c[i]) for ty, c in part) for i in range(n)]
            okey = [tuple(self.group_key(ty, c[i]) for ty, c in order) for i in range(n)]
            kind = w.get("window_expr")
            if kind == "built_in_window_expr":
                if w.get("fun") != "RowNumber":
                    raise NotImplementedError("window function " + str(w.get("fun")))
                out, k = [], 0
                for i in range(n):
                    k = k + 1 if (i > 0 and pkey[i] == pkey[i - 1]) else 1
                    out.append(k)
                names.append(w["name"]), types.append("UInt64"), cols.append(out)
                continue
            if kind != "aggregate_window_expr":
                raise NotImplementedError("window_expr " + str(kind))
            (fn, name, ty, vals), = self.entries([w["aggregate"]], rel)
            if fn == "dc":
                raise NotImplementedError("a distinct count as a window function")
            if fn in ("sum", "avg") and g._type_name(ty) == "Float64":
                raise NotImplementedError("SUM / AVG of Float64")
            unsigned = g._type_name(ty) == "UInt64"
            out = [None] * n
            a = 0
            while a < n:
                b = a
                while b < n and pkey[b] == pkey[a]:
                    b += 1
                rows_seen, live, total, lo, hi = 0, 0, 0, None, None     # the running state of wide_group_ref's rules over rows a .. r

                def value():
                    if fn == "count":
                        return rows_seen if vals is None else live
                    if not live:
                        return None
                    if fn == "sum":
                        return wref.wrapped_sum([total], unsigned)
                    if fn == "avg":
                        return float(wref.wrapped_sum([total])) / float(live)
                    return lo if fn == "min" else hi
                i = a
                while i < b:        # one peer group: rows i .. j - 1
                    j = i + 1
                    while order and j < b and okey[j] == okey[i]:
                        j += 1
                    if not order:
                        j = b
                    for r in range(i, j):
                        rows_seen += 1
                        v = None if vals is None else vals[r]
                        if v is not None:
                            live += 1
                            if fn in ("sum", "avg"):
                                total += v
                            elif fn in ("min", "max"):
                                if _is_f64(ty):                   # A-FO4
                                    lo = v if lo is None else min(lo, v, key=fo.total_key)
                                    hi = v if hi is None else max(hi, v, key=fo.total_key)
                                else:
                                    lo = v if lo is None else wref.minimum([lo, v])
                                    hi = v if hi is None else wref.maximum([hi, v])
                        if "window_frame_excludes_peers" in self.q and order:
                            out[r] = value()
                    if not ("window_frame_excludes_peers" in self.q and order):
                        v = value()
                        for r in range(i, j):
                            out[r] = v
                    i = j
                a = b
            names.append(name), types.append(self.result_type(fn, ty)), cols.append(out)
        return Rel(names + rel.names, types + rel.types, cols + rel.cols)


def leaf_schemas(plan):
    """the field lists of the plan's leaves in leaf order -- depth first, `input` / `left` before `right`, a union's `inputs` in their order --, leaves of one schema once: they are ONE
    relation (the library matches sources to leaves by their column names)"""
    out, seen = [], set()

    def walk(node):
        if node.get("execution_plan") == "memory_exec":
            key = tuple(f["name"] for f in node["schema"]["fields"])
            if key not in seen:
                seen.add(key)
                out.append(node["schema"]["fields"])
        for k in ("input", "left", "right"):
            if isinstance(node.get(k), dict):
                walk(node[k])
        for x in node.get("inputs") or ():
            walk(x)
    walk(plan)
    return out


def run_plan(plan, tables, quirks=frozenset()):
    """-> (names, types, rows) of `plan` over `tables` (one {column: [values]} per leaf, in leaf order: depth first, `left` before `right`; leaves of one
    schema are one relation and take one table).  Raises generic_ops.ExprError where an expression fails the call, NotImplementedError (naming it)
    for a node or expression outside the dialect."""
    rel = _Interp(tables, quirks).assign(plan).run(plan)
    return rel.names, rel.types, rel.rows()
