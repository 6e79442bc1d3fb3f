"""Plain-Python reference of the scalar functions (flock_amd/csrc/valprog.hpp A-F1..A-F8): each function on Python values, and whole expression
trees by rewriting -- bottom-up, every function node becomes a fresh column that holds its reference values, and what is left goes to
oracle.generic_ops.eval_typed.  NULL in gives NULL out; nothing raises."""
import datetime as _dt
import math
import struct

from oracle.generic_ops import eval_typed, static_type

TS = {"Timestamp": ["Millisecond", None]}
_EPOCH = _dt.datetime(1970, 1, 1)
MS_DAY = 86_400_000

MATH = ("abs", "signum", "floor", "ceil", "round", "trunc", "sqrt")
TRUNC_UNITS = ("second", "minute", "hour", "day", "week", "month", "year")
PART_UNITS = ("year", "month", "day", "hour", "minute", "second", "dow", "doy")
ALIASES = {"character_length": "char_length", "length": "char_length"}


def bits(x):
    """A Float64 as its bit pattern, every NaN as one: what 'bit-identical, NaN as NaN' compares."""
    if x is None:
        return None
    return "nan" if x != x else struct.unpack("<q", struct.pack("<d", x))[0]


def _int_valued(x):   # |x| >= 2^52, +-inf: already an integer (or not a number at all)
    return math.isinf(x) or abs(x) >= 2.0 ** 52


def fn_abs(x):
    return math.fabs(x)


def fn_signum(x):
    """Rust f64::signum: 1.0 for +0.0 and +inf, -1.0 for -0.0 and -inf, NaN for NaN."""
    return x if x != x else math.copysign(1.0, x)


def fn_trunc(x):
    if x != x or _int_valued(x):
        return x
    return math.copysign(float(int(x)), x)      # int() truncates towards zero; the sign of a zero result is the argument's


def fn_floor(x):
    if x != x or _int_valued(x):
        return x
    return math.copysign(float(math.floor(x)), x) if math.floor(x) == 0 else float(math.floor(x))


def fn_ceil(x):
    if x != x or _int_valued(x):
        return x
    return math.copysign(float(math.ceil(x)), x) if math.ceil(x) == 0 else float(math.ceil(x))


def fn_round(x):
    """Halves away from zero, written out: the truncated value, one further from zero when the dropped fraction is at least a half."""
    if x != x or _int_valued(x):
        return x
    t = fn_trunc(x)
    if abs(x - t) >= 0.5:                        # (x - t is exact)
        t += math.copysign(1.0, x)
    return math.copysign(t, x)


def fn_sqrt(x):
    if x != x:
        return x
    if x < 0:
        return math.nan
    return math.sqrt(x)                          # correctly rounded (IEEE); sqrt(-0.0) = -0.0


_MATH = {"abs": fn_abs, "signum": fn_signum, "floor": fn_floor, "ceil": fn_ceil, "round": fn_round, "trunc": fn_trunc, "sqrt": fn_sqrt}


def _when(ms):
    return _EPOCH + _dt.timedelta(milliseconds=ms)


def _ms(d):
    delta = d - _EPOCH
    return (delta.days * MS_DAY) + delta.seconds * 1000 + delta.microseconds // 1000


def date_trunc(unit, ms):
    unit = unit.lower()
    if unit == "second":
        return ms // 1000 * 1000                 # Python's // floors: towards minus infinity before 1970
    if unit == "minute":
        return ms // 60_000 * 60_000
    if unit == "hour":
        return ms // 3_600_000 * 3_600_000
    if unit == "day":
        return ms // MS_DAY * MS_DAY
    d = _when(ms // MS_DAY * MS_DAY)
    if unit == "week":
        return _ms(d - _dt.timedelta(days=d.weekday()))     # weekday(): Monday = 0
    if unit == "month":
        return _ms(d.replace(day=1))
    if unit == "year":
        return _ms(d.replace(month=1, day=1))
    raise ValueError("date_trunc unit " + unit)


def date_part(unit, ms):
    unit = unit.lower()
    d = _when(ms)
    if unit in ("year", "month", "day", "hour", "minute", "second"):
        return getattr(d, unit)
    if unit == "dow":
        return (d.weekday() + 1) % 7             # Sunday = 0
    if unit == "doy":
        return d.timetuple().tm_yday
    raise ValueError("date_part unit " + unit)


def octet_length(s):
    return len(s.encode("utf-8"))


def char_length(s):
    return sum(1 for b in s.encode("utf-8") if (b & 0xC0) != 0x80)


def call(name, args, now_ms=None):
    """One function on Python values (the unit of date_trunc / date_part first)."""
    name = ALIASES.get(name.lower(), name.lower())
    if name == "now":
        return now_ms
    if any(a is None for a in args):
        return None
    if name in _MATH:
        return _MATH[name](args[0])
    if name == "date_trunc":
        return date_trunc(args[0], args[1])
    if name == "date_part":
        return date_part(args[0], args[1])
    if name == "octet_length":
        return octet_length(args[0])
    if name == "char_length":
        return char_length(args[0])
    raise ValueError("function " + name)


def result_type(name):
    name = ALIASES.get(name.lower(), name.lower())
    return "Float64" if name in _MATH else TS if name in ("date_trunc", "now") else "Int32"


def fn(name, *args):
    """The serialised node."""
    return {"physical_expr": "scalar_function_expr", "name": name, "args": list(args), "return_type": result_type(name)}


def lit_utf8(s):
    return {"physical_expr": "literal", "value": {"Utf8": s}}


def rewrite(e, table, types, now_ms=None):
    """(expression without function nodes, table with the function columns added, their types added).  `table`: {column: [values]}."""
    table, types = dict(table), dict(types)
    n = len(next(iter(table.values()))) if table else 0

    def values_of(x):
        rows = [dict(zip(table, r)) for r in zip(*table.values())] if table else []
        return [eval_typed(x, r, types, static_type(x, types)) for r in rows] if n else []

    def walk(x):
        if isinstance(x, list):
            return [walk(y) for y in x]
        if not isinstance(x, dict):
            return x
        if x.get("physical_expr") != "scalar_function_expr":
            return {k: walk(v) for k, v in x.items()}
        name = ALIASES.get((x.get("name") or x.get("fun")).lower(), (x.get("name") or x.get("fun")).lower())
        args = [walk(a) for a in x.get("args", [])]
        cols = []
        for a in args:
            if a.get("physical_expr") == "literal" and isinstance(a["value"], dict) and "Utf8" in a["value"]:
                cols.append([a["value"]["Utf8"]] * n)
            else:
                while a.get("physical_expr") == "cast_expr" and a["cast_type"] == "Utf8":
                    a = a["expr"]
                cols.append(values_of(a))
        out = [call(name, [c[i] for c in cols], now_ms) for i in range(n)]
        new = "#fn%d" % len([c for c in table if c.startswith("#fn")])
        table[new] = out
        types[new] = result_type(name)
        return {"physical_expr": "column", "name": new, "index": len(table) - 1}

    return walk(e), table, types


def eval_rows(e, table, types, now_ms=None, want=None):
    """The value of `e` for every row of `table`."""
    x, t, ty = rewrite(e, table, types, now_ms)
    n = len(next(iter(t.values()))) if t else 0
    rows = [dict(zip(t, r)) for r in zip(*t.values())] if n else []
    return [eval_typed(x, r, ty, want or static_type(x, ty)) for r in rows]
