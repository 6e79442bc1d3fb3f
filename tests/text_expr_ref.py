"""Reference for Utf8-valued expressions (flock_amd/csrc/textsel.hpp A-T1..A-T3), in plain Python over {column: [values, None = NULL]} tables: a Utf8
literal, a Utf8 column (a cast to Utf8 may sit in front), CASE whose branches are such or NULL -- searched (`CASE WHEN cond`) and simple (`CASE base
WHEN value`), nested.  Conditions are what the general evaluator takes: they go to the oracle's typed evaluator through tests/scalar_fn_ref.py."""
import scalar_fn_ref as sref


class TextExprError(Exception):
    pass


def lit_utf8(s):
    return {"physical_expr": "literal", "value": {"Utf8": s}}


def lit_null(kind=None):
    """NULL: untyped (`kind` None), or ScalarValue::<kind>(None)."""
    return {"physical_expr": "literal", "value": None if kind is None else {kind: None}}


def case(whens, els=None, base=None):
    return {"physical_expr": "case_expr", "expr": base, "when_then_expr": [[w, t] for w, t in whens], "else_expr": els}


def _literal(e):
    """(is NULL, kind, value) of a literal node."""
    v = e.get("value")
    kind = None
    if isinstance(v, dict) and len(v) == 1:
        kind, v = next(iter(v.items()))
    return v is None, kind, v


def is_text(e, types):
    """True: text-valued; False: a NULL literal without a type; raises where a branch has another type (A-T1)."""
    tag = e.get("physical_expr")
    if tag == "literal":
        null, kind, v = _literal(e)
        if kind == "Utf8" or isinstance(v, str):
            return True
        if null:
            return False
        raise TextExprError("CASE branches of different types")
    if tag == "column":
        if types[e["name"]] != "Utf8":
            raise TextExprError("CASE branches of different types")
        return True
    if tag == "cast_expr" and e["cast_type"] == "Utf8":
        return is_text(e["expr"], types)
    if tag == "case_expr":
        branches = [t for _, t in e["when_then_expr"]] + ([e["else_expr"]] if e.get("else_expr") else [])
        return any([is_text(b, types) for b in branches])
    raise TextExprError("CASE branches of different types")


def pick(conds, values, els, n):
    """A-T2 over columns: conds[j][i] in (True, False, None), values[j][i] / els[i] in (str, None): the first TRUE wins, then ELSE, then NULL."""
    out = []
    for i in range(n):
        v = els[i] if els is not None else None
        for cj, vj in zip(conds, values):
            if cj[i] is True:
                v = vj[i]
                break
        out.append(v)
    return out


def eval_text(e, table, types):
    """The value of the text-valued expression `e` for every row of `table`: str, or None for NULL ('' is a value)."""
    n = len(next(iter(table.values()))) if table else 0
    tag = e.get("physical_expr")
    if tag == "literal":
        null, _, v = _literal(e)
        return [None if null else v] * n
    if tag == "column":
        return list(table[e["name"]])
    if tag == "cast_expr":
        return eval_text(e["expr"], table, types)
    if tag != "case_expr":
        raise TextExprError("not a text-valued expression: " + str(tag))
    is_text(e, types)
    conds = []
    for w, _ in e["when_then_expr"]:
        c = w if e.get("expr") is None else {"physical_expr": "binary_expr", "left": e["expr"], "op": "Eq", "right": w}
        conds.append(sref.eval_rows(c, table, types, want="Boolean"))    # (every condition for every row, A-V7)
    values = [eval_text(t, table, types) for _, t in e["when_then_expr"]]
    els = eval_text(e["else_expr"], table, types) if e.get("else_expr") else None
    return pick(conds, values, els, n)
