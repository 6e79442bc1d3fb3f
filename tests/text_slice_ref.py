"""Reference for the text slice functions (flock_amd/csrc/textslice.hpp A-SL1..A-SL8) in plain Python over {column: [values, None = NULL]} tables:
split_part, left, right, ltrim, rtrim, btrim of a Utf8 column or of another slice of one -- `str.split`, slicing and `lstrip` / `rstrip` / `strip`, which
work on code points as the functions do.  eval_text also takes what tests/text_expr_ref.py takes (literals, columns, CASE), with slices as branches."""
import scalar_fn_ref as sref
import text_expr_ref as tref

SLICE_FNS = ("split_part", "left", "right", "ltrim", "rtrim", "btrim")


def sl(name, *args, return_type="Utf8"):
    """The serialised call."""
    return {"physical_expr": "scalar_function_expr", "name": name, "args": list(args), "return_type": return_type}


def lit(kind, v):
    return {"physical_expr": "literal", "value": {kind: v}}


def split_part(s, delim, n):
    """Field n (1-based) of s cut at every non-overlapping, leftmost occurrence of delim; '' when there are fewer fields (A-SL2)."""
    assert delim != "" and n >= 1
    parts = s.split(delim)
    return parts[n - 1] if n <= len(parts) else ""


def left(s, n):
    """n >= 0: the first n code points; n < 0: all but the last |n| (A-SL3)."""
    return s[:n] if n >= 0 else s[:max(len(s) + n, 0)]


def right(s, n):
    """n > 0: the last n code points; n < 0: all but the first |n|; n = 0: '' (A-SL4)."""
    if n == 0:
        return ""
    return s[max(len(s) - n, 0):] if n > 0 else s[-n:]


def ltrim(s, chars=" "):
    return s.lstrip(chars) if chars else s


def rtrim(s, chars=" "):
    return s.rstrip(chars) if chars else s


def btrim(s, chars=" "):
    return s.strip(chars) if chars else s


_FN = {"split_part": split_part, "left": left, "right": right, "ltrim": ltrim, "rtrim": rtrim, "btrim": btrim}


def _lit_value(e):
    while e.get("physical_expr") == "cast_expr":
        e = e["expr"]
    assert e.get("physical_expr") == "literal", e
    v = e["value"]
    return next(iter(v.values())) if isinstance(v, dict) else v


def is_slice(e):
    return e.get("physical_expr") == "scalar_function_expr" and e["name"].lower() in SLICE_FNS


def eval_text(e, table, types):
    """The value of the text-valued expression `e` for every row: str, or None for NULL ('' is a value; NULL in gives NULL out, A-SL7)."""
    n = len(next(iter(table.values()))) if table else 0
    tag = e.get("physical_expr")
    if is_slice(e):
        vals = eval_text(e["args"][0], table, types)
        rest = [_lit_value(a) for a in e["args"][1:]]
        f = _FN[e["name"].lower()]
        return [None if v is None else f(v, *rest) for v in vals]
    if tag == "cast_expr":
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
