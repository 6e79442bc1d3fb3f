"""Reference for CAST(x AS Utf8) of integers and Timestamp(ms) (flock_amd/csrc/numtext.hpp A-NT1..A-NT7) in plain Python / numpy over
{column: [values, None = NULL]} tables.  Integers go through str(int); timestamps through numpy.datetime_as_string(..., unit="ms") with the 'T' made a
blank and a '.000' dropped (chrono's NaiveDateTime display).  eval_text also takes what tests/text_slice_ref.py takes -- literals, Utf8 columns, CASE, the
slice functions -- with casts as branches and as the value under a slice."""
import numpy as np

import scalar_fn_ref as sref
import text_expr_ref as tref
import text_slice_ref as slref

TS = sref.TS
TS_MIN = -62167219200000     # 0000-01-01 00:00:00
TS_MAX = 253402300799999     # 9999-12-31 23:59:59.999
INT_TYPES = ("Int32", "Int64", "UInt64")


class CastRangeError(Exception):
    """A Timestamp(ms) outside the years 0000..9999 under cast_expr: the call fails (A-NT4)."""


def cast_utf8(e, try_cast=False):
    return {"physical_expr": "try_cast_expr" if try_cast else "cast_expr", "expr": e, "cast_type": "Utf8"}


def int_text(values):
    return [None if v is None else str(int(v)) for v in values]


def ts_text(values, try_cast=False):
    """'YYYY-MM-DD HH:MM:SS[.mmm]' for every millisecond count; outside the years 0000..9999: None under try_cast, CastRangeError otherwise."""
    vals = list(values)
    inside = [v is not None and TS_MIN <= int(v) <= TS_MAX for v in vals]
    if not try_cast and any(v is not None and not ok for v, ok in zip(vals, inside)):
        raise CastRangeError("a Timestamp(ms) outside the years 0000 to 9999")
    ms = np.array([int(v) if ok else 0 for v, ok in zip(vals, inside)], dtype="int64")
    text = np.datetime_as_string(ms.astype("datetime64[ms]"), unit="ms") if len(ms) else []
    out = []
    for ok, t in zip(inside, text):
        if not ok:
            out.append(None)
            continue
        t = str(t).replace("T", " ")
        out.append(t[:-4] if t.endswith(".000") else t)
    return out


def is_num_cast(e, types):
    """cast_expr / try_cast_expr to Utf8 over something that is not text."""
    if e.get("physical_expr") not in ("cast_expr", "try_cast_expr") or e["cast_type"] != "Utf8":
        return False
    x = e["expr"]
    tag = x.get("physical_expr")
    if tag == "column":
        return types[x["name"]] != "Utf8"
    if tag == "literal":
        v = x.get("value")
        v = next(iter(v.values())) if isinstance(v, dict) and v else v
        return v is not None and not isinstance(v, str)
    if tag in ("cast_expr", "try_cast_expr"):
        return x["cast_type"] != "Utf8" or is_num_cast(x, types)
    return tag not in ("case_expr",) and not slref.is_slice(x)


def operand_type(x, types):
    if x.get("physical_expr") == "column":
        return types[x["name"]]
    if x.get("physical_expr") in ("cast_expr", "try_cast_expr"):
        return x["cast_type"]
    if x.get("physical_expr") == "scalar_function_expr":
        return sref.result_type((x.get("name") or x.get("fun")).lower())
    from oracle.generic_ops import static_type
    return static_type(x, types)


def eval_text(e, table, types):
    """The value of the text-valued expression `e` for every row: str, or None for NULL."""
    n = len(next(iter(table.values()))) if table else 0
    tag = e.get("physical_expr")
    if is_num_cast(e, types):
        x = e["expr"]
        ty = operand_type(x, types)
        vals = list(table[x["name"]]) if x.get("physical_expr") == "column" else sref.eval_rows(x, table, types)
        if ty == TS:
            return ts_text(vals, try_cast=tag == "try_cast_expr")
        assert ty in INT_TYPES, ty
        return int_text(vals)
    if slref.is_slice(e):
        vals = eval_text(e["args"][0], table, types)
        rest = [slref._lit_value(a) for a in e["args"][1:]]
        f = slref._FN[e["name"].lower()]
        return [None if v is None else f(v, *rest) for v in vals]
    if tag in ("cast_expr", "try_cast_expr"):
        return eval_text(e["expr"], table, types)
    if tag == "case_expr":
        conds = []
        for w, _ in e["when_then_expr"]:
            c = w if e.get("expr") is None else {"physical_expr": "binary_expr", "left": e["expr"], "op": "Eq", "right": w}
            conds.append(sref.eval_rows(c, table, types, want="Boolean"))
        values = [eval_text(t, table, types) for _, t in e["when_then_expr"]]
        els = eval_text(e["else_expr"], table, types) if e.get("else_expr") else None
        return tref.pick(conds, values, els, n)
    return tref.eval_text(e, table, types)
