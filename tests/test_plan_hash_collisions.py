"""Crafted hash collisions for the open-addressing tables of the generic operators (relops.hip, distinct.hip), through ExecutionContext + collect,
against the CPU references (oracle.generic_ops, tests/count_distinct_ref.py, semi_anti_ref.py, wide_group_ref.py), exactly and row for row.

Random and NEXMark-shaped keys never reach the branches that decide correctness only when two DIFFERENT keys meet in a table: a slot whose 32-bit tag
agrees while the key differs, a probe run that wraps from slot cap - 1 to 0 or passes many foreign slots, the 8 probes of the workgroup table, the
chains of the one-workgroup kernels, the probe cut-offs.  tests/hash_craft.py makes such inputs (its claims are proven on the CPU by
tests/test_hash_craft.py, its mirrors of the hashes pinned to the kernel text by tests/test_source_constants.py); every test here feeds its input
twice, whole and in batches of 2500 rows, and asserts by name that the kernel it is about ran."""
import functools
import os
import re

import numpy as np
import pytest

import count_distinct_ref as dref
import hash_craft as hc
import test_plan_composite_keys as K
import test_plan_count_distinct as D
import test_plan_semi_anti as S
import test_plan_wide_group_by as W
import wide_group_ref as wref
from oracle import generic_ops as g
from semi_anti_ref import semi_anti_table, table_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 2500


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _run(gpu, plan, feeds, chunk=None, ctx=None):
    """feeds: per leaf (table, cols) -> (the output's rows, the names of the kernels that ran)"""
    from flock_amd.runtime import ExecutionContext, collect
    own = ctx is None
    ctx = ctx or ExecutionContext([plan], gpu=gpu)
    gpu.profile_reset()
    gpu.profile(True)
    try:
        out = collect(ctx, [[K._batches(t, chunk or max(1, len(t[cols[0][0]])), cols)] for t, cols in feeds])[0]
        ran = set(gpu.profile_read())
    finally:
        gpu.profile(False)
        if own:
            ctx.close()
    rows = []
    for rb in out:
        rows += K._pyrows(rb)
    return rows, ran


def _srt(rows):
    return sorted(rows, key=lambda r: tuple((0, 0) if v is None else (1, v) for v in r))


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


# ------------------------------------------------------------------ (a) (b): composite keys whose LAST Int64 column is steered
# (tag, low 24 bits of the hash) of the eight clusters: tags 0 and 0xFFFFFFFF, homes cap - 1 (0xFFFFFF: the run wraps to slot 0) and 0, two clusters
# on neighbouring homes (one run), 0x003FFF = the last slot of a 16384-slot table as well
CLUSTERS = [(0, 0xFFFFFF), (0xFFFFFFFF, 0), (0x9E3779B1, 0x123456), (0, 0x123457), (0x7FFFFFFF, 0xABCDEF), (0x80000000, 0x00FFFF), (1, 0x003FFF),
            (0xFFFFFFFF, 0x800000)]
ACOLS = [("a", "Int64"), ("b", "Int64"), ("s", "Utf8"), ("bs", "Int64"), ("v", "Int64"), ("f", "Float64")]
PCOLS = [("a_r", "Int64"), ("b_r", "Int64"), ("s_r", "Utf8"), ("bs_r", "Int64"), ("p", "Int64")]


def _first_a(m):
    """the first Int64 column of tuple m: few values, so that it never tells two tuples of a cluster apart on its own; some NULL"""
    return None if m % 9 == 4 else (m % 7 - 3) * 10**12


def _first_s(m):
    return None if m % 11 == 5 else ["", "a", "ab", "name-%d" % (m % 5), "x" * 17, "w" * 70][m % 6]


def _tuple(m, target):
    """(a, b, s, bs): b makes (a, b) hash to `target`, bs makes (s, bs) hash to it"""
    a, s = _first_a(m), _first_s(m)
    return (a, hc.steer_last_i64(hc.prefix_hash([a]), target), s, hc.steer_last_i64(hc.prefix_hash([s]), target))


def _cluster_tuples(lo, hi, tag_xor=0):
    return [_tuple(m, ((tag ^ tag_xor) << 32) | (m << 24) | low) for tag, low in CLUSTERS for m in range(lo, hi)]


def _behind_tuples(per_cluster):
    """ordinary tuples (tags of their own) whose homes lie 1 .. 70 slots behind a cluster's: their probes walk through it"""
    out = []
    for c, (_, low) in enumerate(CLUSTERS):
        for j in range(per_cluster):
            t = (hc._tag_of(1000 * c + j) << 32) | ((j & 0xFF) << 24) | ((low + 1 + (j * 7) % 70) & 0xFFFFFF)
            out.append(_tuple(200 + j, t))
    return out


@functools.lru_cache(maxsize=None)
def _composite():
    """-> (the GROUP BY table of about 6000 rows, its distinct tuples).  Eight clusters of 64 tuples, each tuple two to five times, 40 tuples behind
    every cluster, ordinary tuples; rows shuffled."""
    r = np.random.default_rng(1601)
    present = _cluster_tuples(0, 64)
    tuples = present + _behind_tuples(40)
    for j in range(1400):
        a = None if j % 50 == 7 else int(r.integers(-2**62, 2**62))
        s = None if j % 50 == 9 else "o%d" % r.integers(0, 10**6)
        tuples.append((a, int(r.integers(-2**62, 2**62)), s, int(r.integers(-2**62, 2**62))))
    rows = []
    for k, tp in enumerate(tuples):
        rows += [tp] * (int(r.integers(2, 6)) if k < len(present) else int(r.integers(1, 4)))
    rows = [rows[i] for i in r.permutation(len(rows))]
    n = len(rows)
    t = {"a": [x[0] for x in rows], "b": [x[1] for x in rows], "s": [x[2] for x in rows], "bs": [x[3] for x in rows],
         "v": [int(x) for x in r.integers(-10**6, 10**6, n)], "f": [None if x < 0.2 else float(int(x * 1000)) for x in r.random(n)]}
    assert 5000 < n < 7000 and hc.pow2_at_least(2 * n) == 16384
    return t, tuples


SHAPES = {"i64_i64": ["a", "b"], "utf8_i64": ["s", "bs"]}
AGG3 = [("count", None, "UInt64"), ("sum", "v", "Int64"), ("min", "v", "Int64")]
AGG9 = [("count", None), ("count", "v"), ("count", "f"), ("min", "v"), ("max", "v"), ("sum", "v"), ("min", "f"), ("max", "f"), ("min", "bs")]
assert W.n_accs(AGG9) == 9


def test_the_composite_clusters_collide_as_claimed():
    """(CPU) every cluster of the GROUP BY table: 64 different tuples, ONE tag and ONE home under key_tuple_hash, in both key shapes"""
    t, tuples = _composite()
    for c, (tag, low) in enumerate(CLUSTERS):
        mine = tuples[64 * c:64 * (c + 1)]
        for cols in ((0, 1), (2, 3)):
            keys = [(tp[cols[0]], tp[cols[1]]) for tp in mine]
            hs = [hc.key_tuple_hash(k) for k in keys]
            assert len(set(keys)) == 64 and {h >> 32 for h in hs} == {tag} and {h & 0xFFFFFF for h in hs} == {low}
    assert any(tp[0] is None for tp in tuples[:64]) and any(tp[2] is None for tp in tuples[:64])
    assert -2**63 not in t["b"] and -2**63 not in t["bs"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_composite_group_by_on_tag_clusters(gpu, shape):
    """key_codes_insert_kernel: 64 tuples per cluster share the slot tag AND the home slot (tags 0 and 0xFFFFFFFF, a cluster at slot cap - 1 whose run
    wraps), some with a NULL first column (its marker enters the hash).  Accepting a slot on its tag alone would merge a cluster into one group.
    COUNT(*), SUM, MIN: the groups AND their order of first appearance; the same under SELECT DISTINCT and under nine accumulators."""
    keys = SHAPES[shape]
    t, tuples = _composite()
    want = K._oracle_rows(t, keys, AGG3)
    want_distinct = K._oracle_rows(t, keys, [])
    assert len(want) == len(tuples) == len(want_distinct)
    want9 = wref.aggregate(t, keys, AGG9, dict(ACOLS))
    for chunk in (None, CHUNK):
        got, ran = _run(gpu, K._group_plan(keys, AGG3, ACOLS), [(t, ACOLS)], chunk)
        assert "key_codes_insert_kernel" in ran, sorted(ran)
        assert got == want, (shape, chunk, len(got), len(want))
        got, ran = _run(gpu, K._group_plan(keys, [], ACOLS), [(t, ACOLS)], chunk)
        assert "key_codes_insert_kernel" in ran, sorted(ran)
        assert got == want_distinct, (shape, chunk, len(got))
        got, ran = _run(gpu, W.whole_plan(keys, AGG9, cols=ACOLS), [(t, ACOLS)], chunk)
        assert "key_codes_insert_kernel" in ran and "wide_group_kernel" in ran, sorted(ran)
        assert wref.same_rows(wref.sort_rows(got, 2), wref.sort_rows(want9, 2)), (shape, chunk, len(got))


@functools.lru_cache(maxsize=None)
def _composite_probe():
    """20000 probe rows: tuples of the build side; absent tuples of the SAME tag and home (members 64 .. 127 of every cluster: the first column of
    each is a present tuple's); absent tuples of a foreign tag and the same home; rows whose first key column is NULL."""
    r = np.random.default_rng(1602)
    _, tuples = _composite()
    absent = _cluster_tuples(64, 128) + _cluster_tuples(0, 64, tag_xor=0x5A5A5A5A)
    assert not set(absent) & set(tuples)
    pool = tuples + absent
    pick = np.where(r.random(20_000) < 0.5, r.integers(0, len(tuples), 20_000), len(tuples) + r.integers(0, len(absent), 20_000))
    rows = [pool[i] for i in pick]
    return {"a_r": [x[0] for x in rows], "b_r": [x[1] for x in rows], "s_r": [x[2] for x in rows], "bs_r": [x[3] for x in rows], "p": list(range(20_000))}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("jt", ["Inner", "Semi", "Anti"])
def test_composite_joins_probe_tag_clusters(gpu, shape, jt):
    """key_codes_probe_kernel: probe tuples that are absent but carry a present cluster's tag and home must not match, nor may NULL-keyed ones."""
    build, _ = _composite()
    probe = _composite_probe()
    on = [(k, k + "_r") for k in SHAPES[shape]]
    if jt == "Inner":
        plan = K._join_plan(ACOLS, PCOLS, on)
        feeds = [(build, ACOLS), (probe, PCOLS)]
        want = _srt(g.rows(g.hash_join_inner(build, probe, on)))
    else:
        ron = [(b, a) for a, b in on]
        plan = S._semi_plan(jt, ron, lcols=PCOLS, rcols=ACOLS)
        feeds = [(probe, PCOLS), (build, ACOLS)]
        want = table_rows(semi_anti_table(probe, build, ron, jt == "Anti"), [c for c, _ in PCOLS])
    assert 4000 < len(want)
    for chunk in (None, CHUNK):
        got, ran = _run(gpu, plan, feeds, chunk)
        assert "key_codes_insert_kernel" in ran and "key_codes_probe_kernel" in ran, sorted(ran)
        assert (_srt(got) if jt == "Inner" else got) == want, (shape, jt, chunk, len(got), len(want))


# ------------------------------------------------------------------ (c) hashed GROUP BY on one 64-bit key: both instantiations of group_insert_n_kernel
GCOLS = [("k", "Int64"), ("x", "Int64"), ("f", "Float64"), ("v", "Int64")]
QCOLS = [("p", "Int32"), ("q", "Int32"), ("x", "Int64"), ("f", "Float64"), ("v", "Int64")]
GAGG = [("count", "x", "UInt64"), ("min", "f", "Float64"), ("max", "f", "Float64")]


def _lds_geometry(width):
    """(rows per workgroup, rows from which the workgroup-table instantiation runs) for `width` accumulators, read from group_by_key64_n"""
    with open(os.path.join(ROOT, "flock_amd", "csrc", "relops.hip")) as f:
        src = f.read()
    m = re.search(r"const uint32_t lds_slots = width <= (\d+) \? (\d+)u : (\d+)u;", src)
    per = re.search(r"const int64_t rows_per_wg = \(int64_t\)lds_slots \* (\d+);", src)
    sw = re.search(r"if \(rows >= rows_per_wg \* (\d+) && sp\.n > 0\) \{", src)
    assert m and per and sw, "group_by_key64_n no longer states its workgroup-table geometry in the form the test reads"
    slots = int(m.group(2)) if width <= int(m.group(1)) else int(m.group(3))
    return slots * int(per.group(1)), slots * int(per.group(1)) * int(sw.group(1))


@functools.lru_cache(maxsize=None)
def _group_keys(n):
    """n rows of Int64 keys.  Rows 0 .. 11 carry ONE key of a 40-key cluster (the first wave's combine: twelve of its 64 rows share its first row's
    key); every workgroup's run of rows holds 40 keys that share their low 24 hash bits (the ninth and later miss the 8 probes of the workgroup
    table and go to the global one); a second cluster sits on the LAST slot of every table; ordinary keys, some homed just behind the clusters."""
    r = np.random.default_rng(1603 + n)
    per_wg, _ = _lds_geometry(len(GAGG))
    c1 = hc.home_cluster(0x5A5A5A, 40)
    c2 = hc.tag_cluster(0xFFFFFFFF, 0xFFFFFF, 40)
    near = hc.behind(0x5A5A5A, 3, 30) + hc.behind(0xFFFFFF, 1, 30) + hc.behind(0x5A5A5A, 41, 10)
    ordinary = [int(x) for x in r.integers(-2**62, 2**62, 1500)]
    keys = []
    for base in range(0, n, per_wg):
        m = min(per_wg, n - base)
        block = [(c1 + c2 + near)[i] for i in r.integers(0, 150, m // 4)] + [ordinary[i] for i in r.integers(0, 1500, m - m // 4)]
        block = [block[i] for i in r.permutation(m)]
        keys += block
    keys[:12] = [c1[0]] * 12
    keys[12:52] = c1[1:] + [c2[0]]
    assert len(keys) == n
    return keys


def _group_table(n, pair):
    r = np.random.default_rng(7 * n)
    keys = _group_keys(n)
    t = {"x": [None if u < 0.3 else int(u * 1000) for u in r.random(n)], "f": [float(int(u)) / 8 for u in r.integers(-10**6, 10**6, n)],
         "v": [int(u) for u in r.integers(-99, 99, n)]}
    if pair:   # the two Int32 columns together ARE the 64-bit key (pack_pair_kernel: first column high, second low)
        t["p"], t["q"] = [_i32(k >> 32) for k in keys], [_i32(k) for k in keys]
    else:
        t["k"] = keys
    return t


def test_the_group_by_row_counts_lie_on_either_side_of_the_switch():
    per_wg, switch = _lds_geometry(len(GAGG))
    assert 9_000 < switch <= 40_000 and per_wg >= 64
    keys = _group_keys(40_000)
    for base in range(0, 40_000 - per_wg, per_wg):          # every whole run of rows: far more keys of one home than the workgroup table's 8 probes reach
        block = set(keys[base:base + per_wg])
        assert all(sum(1 for k in block if hc.mix64(k) & 0xFFFFFF == low) >= 30 for low in (0x5A5A5A, 0xFFFFFF)), base
    assert len({hc.mix64(k) & 0xFFFFFF for k in keys[:52]}) == 2 and len(set(keys[:52])) == 41


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True], ids=["int64", "int32_pair"])
@pytest.mark.parametrize("n", [9_000, 40_000])
def test_hashed_group_by_with_keys_that_share_their_home(gpu, n, pair):
    """group_insert_n_kernel: 9000 rows run <false> (every row to the global table), 40000 rows <true> (a workgroup table of 8 probes first; the
    switch is read from the source).  COUNT of a column with NULLs (the `seen` counters), MIN / MAX of Float64."""
    t = _group_table(n, pair)
    cols, keys = (QCOLS, ["p", "q"]) if pair else (GCOLS, ["k"])
    want = _srt(K._oracle_rows(t, keys, GAGG))
    for chunk in (None, CHUNK):
        got, ran = _run(gpu, K._group_plan(keys, GAGG, cols), [(t, cols)], chunk)
        assert "group_insert_n_kernel" in ran and "dense_group_kernel" not in ran and "key_codes_insert_kernel" not in ran, sorted(ran)
        assert _srt(got) == want, (n, pair, chunk, len(got), len(want))


# ------------------------------------------------------------------ (d) COUNT(DISTINCT)
DCOLS = [("g", "Int32"), ("l", "Int64"), ("i", "Int32"), ("s", "Utf8")]


def _dc(gpu, t, keys, arg, ctx=None, chunk=None):
    plan = D.whole_plan(keys, [("dc", arg)], cols=DCOLS)
    got, ran = _run(gpu, plan, [(t, DCOLS)], chunk, ctx=ctx)
    want = dref.sort_rows(dref.aggregate(t, keys, [("dc", arg)]), len(keys))
    return dref.sort_rows(got, len(keys)), want, ran


def _dc_table(values, seed):
    """every value at least twice, rows shuffled; the columns no test reads hold zeros"""
    r = np.random.default_rng(seed)
    rows = list(values) * 2 + [values[i] for i in r.integers(0, len(values), len(values) // 2)]
    rows = [rows[i] for i in r.permutation(len(rows))]
    n = len(rows)
    return {"g": [0] * n, "l": [0] * n, "i": [0] * n, "s": [""] * n}, rows


@pytest.mark.gpu
def test_count_distinct_ungrouped_over_tag_clusters_and_again_with_a_hint_sized_table(gpu):
    """distinct.hip distinct_insert_kernel: four tag clusters of 128 Int64 values (one tag, one home; tags 0 and 0xFFFFFFFF, home cap - 1), every value
    repeated.  A kernel that compared the tag and not the value would count 1 per cluster.  The second execute on the same context -- other
    clusters -- meets a table sized from the first one's count (.pairs_hint)."""
    from flock_amd.runtime import ExecutionContext
    r = np.random.default_rng(1604)
    specs = [[(0, 0xFFFFFF), (0xFFFFFFFF, 0), (0x13579BDF, 0x0F0F0F), (0x13579BDF, 0x0F0F10)], [(0xFFFFFFFF, 0xFFFFFF), (0, 0), (7, 0x777777), (8, 0x777777)]]
    for chunk in (None, CHUNK):
        ctx = ExecutionContext([D.whole_plan([], [("dc", "l")], cols=DCOLS)], gpu=gpu)
        try:
            for k, spec in enumerate(specs):
                values = [v for tag, low in spec for v in hc.tag_cluster(tag, low, 128)]
                values += [v for _, low in spec for v in hc.behind(low, 5, 20)] + [int(x) for x in r.integers(-2**62, 2**62, 500)] + [None]
                t, rows = _dc_table(values, 10 + k)
                t["l"] = rows
                got, want, ran = _dc(gpu, t, [], "l", ctx=ctx, chunk=chunk)
                assert "distinct_insert_kernel" in ran, sorted(ran)
                assert got == want == [(len(set(values)) - 1,)], (chunk, k, got, want)
        finally:
            ctx.close()


@pytest.mark.gpu
def test_count_distinct_grouped_over_pairs_of_identical_hashes(gpu):
    """200 groups whose first rows appear in group order (the composite ids are the group numbers).  Every group holds the value that gives its
    (group, value) pair the SAME 64-bit hash as every other group's, every second group a second value whose pair shares tag and home with the
    first: a slot that agrees in tag and group still has to agree in value.  Each group's count is exact.
    (What these inputs cannot show is a kernel that drops the GROUP comparison and keeps the value's: that needs ONE value in two groups whose
    pairs share tag and home -- about 45 agreeing hash bits at a fixed difference of the hashed words, which neither inversion nor search gives.
    The small values 0 .. 39, which every group holds, are there for the day a hash change makes them meet.)"""
    r = np.random.default_rng(1605)
    x0, x1 = hc.tag_cluster(0xFFFFFFFF, 0xFFFFFF, 2)
    first = hc.same_hash_pairs(x0, range(200))
    pairs = first + hc.same_hash_pairs(x1, range(0, 200, 2))
    assert len({hc.distinct_pair_hash(q, v) for q, v in first}) == 1 and len({hc.distinct_pair_hash(q, v) >> 32 for q, v in pairs}) == 1
    rest = pairs * 2 + [(int(q), int(v)) for q, v in zip(r.integers(0, 200, 3000), r.integers(0, 40, 3000))] + [(q, None) for q in range(0, 200, 7)]
    rows = first + [rest[i] for i in r.permutation(len(rest))]
    n = len(rows)
    t = {"g": [q * 3 - 250 for q, _ in rows], "l": [v for _, v in rows], "i": [0] * n, "s": [""] * n}
    for chunk in (None, CHUNK):
        got, want, ran = _dc(gpu, t, ["g"], "l", chunk=chunk)
        assert "distinct_insert_kernel" in ran and "key_codes_insert_kernel" in ran, sorted(ran)
        assert got == want and len(got) == 200, (chunk, [p for p in zip(got, want) if p[0] != p[1]][:5])


@pytest.mark.gpu
@pytest.mark.parametrize("arg", ["i", "s"])
def test_count_distinct_over_searched_home_clusters(gpu, arg):
    """An Int32 argument (hashed sign-extended) and a Utf8 argument (counted over the codes of utf8_codes_build_kernel's dictionary): neither can be
    steered, so the clusters -- 64 Int32 values, 16 and more strings with last-byte twins and two lengths -- are found by search at the table's
    exact size: 6000 rows, 16384 slots."""
    r = np.random.default_rng(1606)
    n = 6000
    cap = hc.pow2_at_least(2 * n)
    if arg == "i":
        values = [v for c in hc.search_i32(cap, 64, count=6) for v in c] + [int(x) for x in r.integers(-2**31, 2**31, 1500)]
    else:
        values = [s for c in hc.search_utf8(cap, 16, count=6) for s in c] + ["t%d" % x for x in r.integers(0, 10**9, 1500)] + [""]
    rows = values * 2 + [None] * 50
    rows += [values[i] for i in r.integers(0, len(values), n - len(rows))]
    rows = [rows[i] for i in r.permutation(n)]
    t = {"g": [0] * n, "l": [0] * n, "i": [0] * n, "s": [""] * n}
    t[arg] = rows
    for chunk in (None, CHUNK):
        got, want, ran = _dc(gpu, t, [], arg, chunk=chunk)
        assert "distinct_insert_kernel" in ran and ("utf8_codes_build_kernel" in ran) == (arg == "s"), sorted(ran)
        assert got == want == [(len(set(values)),)], (arg, chunk, got, want)


# ------------------------------------------------------------------ (e) (f) (g): joins and semi / anti joins on one integer key
def _jcols(lt, rt):
    return [("a", lt), ("x", "Int32")], [("b", rt), ("y", "Int64")]


def _int_clusters(ktype, cap, size, spare):
    """two clusters of `size` keys plus `spare` more keys of each cluster's home that stay off the build side.  Int64: home cap - 1 (the run wraps) and
    home 0, in every table; Int32: found by search for a table of exactly `cap` slots."""
    if ktype == "Int64":
        lows = (0xFFFFFF, 0)
        return [hc.home_cluster(low, size) for low in lows], [hc.home_cluster(low, spare, first=size) for low in lows], \
               [hc.behind(low, size, 30) for low in lows]
    found = hc.search_i32(cap, size + spare, count=2)
    return [c[:size] for c in found], [c[size:] for c in found], [[], []]


def _join_sides(ktypes, n_build, n_probe, size, seed, cap=None):
    """-> (unique build keys, probe keys): clusters of `size` on the build side; probe keys present, absent but homed inside a cluster, absent and
    homed at the slot after its end, and absent ordinary ones."""
    r = np.random.default_rng(seed)
    narrow = "Int32" in ktypes
    cap = cap or hc.pow2_at_least(2 * n_build)
    clusters, spare, after = _int_clusters("Int32" if narrow else "Int64", cap, size, size // 4)
    lo, hi = (-2**31, 2**31) if narrow else (-2**62, 2**62)
    taken = set(v for c in clusters + spare + after for v in c)
    ordinary = []
    while len(ordinary) < n_build - 2 * size:
        v = int(r.integers(lo, hi))
        if v not in taken:
            taken.add(v)
            ordinary.append(v)
    build = [v for c in clusters for v in c] + ordinary
    build = [build[i] for i in r.permutation(n_build)]
    absent = [v for c in spare + after for v in c] + [int(x) for x in r.integers(lo, hi, 500) if int(x) not in taken]
    in_cluster = [v for c in clusters for v in c]
    probe = [in_cluster[i] for i in r.integers(0, len(in_cluster), n_probe // 4)] + [absent[i] for i in r.integers(0, len(absent), n_probe // 4)]
    probe += [build[i] for i in r.integers(0, n_build, n_probe - len(probe))]
    probe = [probe[i] for i in r.permutation(n_probe)]
    return build, probe, in_cluster


def _join_tables(build, probe, seed):
    r = np.random.default_rng(seed)
    return ({"a": build, "x": [int(v) for v in r.integers(-9, 9, len(build))]}, {"b": probe, "y": [int(v) for v in r.integers(-2**40, 2**40, len(probe))]})


@pytest.mark.gpu
@pytest.mark.parametrize("ktypes", [("Int64", "Int64"), ("Int32", "Int32"), ("Int32", "Int64")], ids=["i64", "i32", "i32_x_i64"])
def test_hashed_join_through_home_clusters(gpu, ktypes):
    """join_hash_build_kernel, 5000 build rows (above the one-workgroup join), 20000 probe rows.  Int64: clusters of 200 keys at home cap - 1 and at
    home 0; Int32 (and Int32 x Int64): clusters of 100 found by search.  Unique build keys are probed by join_hash_probe_flag_kernel; the same plan
    instance, a third of the cluster keys twice on the build side, by join_hash_probe_kernel.  A lookup that gave up at the first occupied slot
    holding another key would lose every cluster key that is not at its home."""
    from flock_amd.runtime import ExecutionContext
    size = 200 if ktypes == ("Int64", "Int64") else 100
    build, probe, in_cluster = _join_sides(ktypes, 5000, 20_000, size, 1607)
    lcols, rcols = _jcols(*ktypes)
    plan = K._join_plan(lcols, rcols, [("a", "b")])
    dup, members = list(build), set(in_cluster)
    at = [i for i, v in enumerate(build) if v not in members]
    for j, v in enumerate(in_cluster[::3]):
        dup[at[j]] = v                                          # a third of the cluster keys a second time, in place of ordinary keys
    for chunk in (None, CHUNK):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            for keys, kernel, sibling in ((build, "join_hash_probe_flag_kernel", "join_hash_probe_kernel"), (dup, "join_hash_probe_kernel", None)):
                left, right = _join_tables(keys, probe, 3)
                got, ran = _run(gpu, plan, [(left, lcols), (right, rcols)], chunk, ctx=ctx)
                assert "join_hash_build_kernel" in ran and kernel in ran and sibling not in ran and "join_tiny_kernel" not in ran, sorted(ran)
                want = _srt(g.rows(g.hash_join_inner(left, right, [("a", "b")])))
                assert _srt(got) == want and 10_000 < len(want), (ktypes, chunk, kernel, len(got), len(want))
        finally:
            ctx.close()


def _tiny_sides(seed):
    """3000 build rows, 10000 probe rows: clusters of 256 keys at slot kTinySlots - 1 (one tag) and of 200 at slot 0, a third of the cluster keys
    twice on the build side (chains)"""
    r = np.random.default_rng(seed)
    clusters = [hc.tag_cluster(0xFFFFFFFF, 0xFFFFFF, 256), hc.home_cluster(0, 200)]
    spare = [hc.home_cluster(0xFFFFFF, 60, first=5000), hc.home_cluster(0, 60, first=6000), hc.behind(0xFFFFFF, 256, 30), hc.behind(0, 200, 30)]
    in_cluster = [v for c in clusters for v in c]
    build = in_cluster + in_cluster[::3]
    build += [int(x) for x in r.integers(-2**62, 2**62, 3000 - len(build))]
    build = [build[i] for i in r.permutation(3000)]
    absent = [v for c in spare for v in c]
    probe = [in_cluster[i] for i in r.integers(0, len(in_cluster), 3000)] + [absent[i] for i in r.integers(0, len(absent), 3000)]
    probe += [build[i] for i in r.integers(0, 3000, 4000)]
    return build, [probe[i] for i in r.permutation(10_000)]


@pytest.mark.gpu
def test_one_workgroup_join_with_chains_inside_clusters(gpu):
    """join_tiny_kernel: a table of kTinySlots = 8192 slots in LDS; 256 keys of one tag at slot 8191 (the run wraps), 200 at slot 0, duplicates
    inside the clusters (a key's build rows come out in chain order: compared as sorted rows)."""
    build, probe = _tiny_sides(1608)
    lcols, rcols = _jcols("Int64", "Int64")
    left, right = _join_tables(build, probe, 4)
    want = _srt(g.rows(g.hash_join_inner(left, right, [("a", "b")])))
    assert len({hc.mix64(v) & 8191 for v in hc.tag_cluster(0xFFFFFFFF, 0xFFFFFF, 256)}) == 1 and len(want) > 8000
    for chunk in (None, CHUNK):
        got, ran = _run(gpu, K._join_plan(lcols, rcols, [("a", "b")]), [(left, lcols), (right, rcols)], chunk)
        assert "join_tiny_kernel" in ran and "join_hash_build_kernel" not in ran, sorted(ran)
        assert _srt(got) == want, (chunk, len(got), len(want))


SLCOLS = [("a", "Int64"), ("x", "Int32")]
SRCOLS = [("b", "Int64"), ("y", "Int64")]


def _semi_check(gpu, jt, left, right, lcols, rcols, kernels, absent_kernels):
    plan = S._semi_plan(jt, [("a", "b")], lcols=lcols, rcols=rcols)
    want = table_rows(semi_anti_table(left, right, [("a", "b")], jt == "Anti"), [c for c, _ in lcols])
    assert 0 < len(want) < len(left["a"])
    for chunk in (None, CHUNK):
        got, ran = _run(gpu, plan, [(left, lcols), (right, rcols)], chunk)
        assert all(k in ran for k in kernels) and not any(k in ran for k in absent_kernels), sorted(ran)
        assert got == want, (jt, chunk, len(got), len(want))


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
def test_one_workgroup_semi_and_anti_join_with_null_left_keys(gpu, jt):
    """semi_tiny_kernel: the clusters of the one-workgroup join as the right side's key set; left keys absent but homed inside and just behind the
    clusters; NULL left keys (dropped by Semi, kept by Anti)."""
    build, probe = _tiny_sides(1609)
    left = {"a": [None if i % 17 == 3 else v for i, v in enumerate(probe)], "x": [i % 7 for i in range(len(probe))]}
    right = {"b": build, "y": list(range(len(build)))}
    _semi_check(gpu, jt, left, right, SLCOLS, SRCOLS, ["semi_tiny_kernel"], ["semi_set_build_kernel", "semi_probe_bitmap_flag_kernel"])
    assert (jt == "Anti") == any(v is None for v in semi_anti_table(left, right, [("a", "b")], jt == "Anti")["a"])


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
@pytest.mark.parametrize("ktype", ["Int64", "Int32"])
def test_hashed_semi_and_anti_join_through_home_clusters(gpu, jt, ktype):
    """semi_set_build_kernel + semi_probe_set_flag_kernel<kI32 / !kI32, kAnti>: 6000 right rows with repeats whose keys no bitmap covers, 30000 left
    rows; the clusters of the hashed join (Int64: 200 keys at home cap - 1 and at 0; Int32: 100 by search)."""
    r = np.random.default_rng(1610)
    size = 200 if ktype == "Int64" else 100
    keys, probe, _ = _join_sides((ktype, ktype), 4000, 30_000, size, 1611, cap=hc.pow2_at_least(2 * 6000))
    right_keys = keys + [keys[i] for i in r.integers(0, 4000, 2000)]
    right_keys = [right_keys[i] for i in r.permutation(6000)]
    probe = [None if i % 19 == 5 else v for i, v in enumerate(probe)]
    lcols, rcols = [("a", ktype), ("x", "Int32")], [("b", ktype), ("y", "Int64")]
    left = {"a": probe, "x": [i % 11 for i in range(30_000)]}
    right = {"b": right_keys, "y": list(range(6000))}
    _semi_check(gpu, jt, left, right, lcols, rcols, ["semi_set_build_kernel", "semi_probe_set_flag_kernel"], ["semi_tiny_kernel", "semi_probe_bitmap_flag_kernel"])


# ------------------------------------------------------------------ (h) one Utf8 key; DISTINCT (Int32, Utf8)
UCOLS = [("s", "Utf8"), ("v", "Int64"), ("f", "Float64")]
URCOLS = [("s_r", "Utf8"), ("y", "Int64")]


@functools.lru_cache(maxsize=None)
def _utf8_sides():
    """6000 build rows (a dictionary of 16384 slots): four searched clusters -- strings that differ only in their last byte, strings of two lengths
    -- of which every fifth member stays off the build side; 8000 probe rows with present strings, those absent members, and other absent ones."""
    r = np.random.default_rng(1612)
    n = 6000
    found = hc.search_utf8(hc.pow2_at_least(2 * n), 16, count=4)
    held = [s for c in found for k, s in enumerate(c) if k % 5 != 4]
    off = [s for c in found for k, s in enumerate(c) if k % 5 == 4]
    values = held + ["u%d" % x for x in r.integers(0, 10**9, 1800)] + ["", "é", "w" * 70]
    rows = values * 2
    rows += [values[i] for i in r.integers(0, len(values), n - len(rows))]
    build = [rows[i] for i in r.permutation(n)]
    absent = off + ["u%dx" % x for x in r.integers(0, 10**9, 300)]
    probe = [held[i] for i in r.integers(0, len(held), 2000)] + [absent[i] for i in r.integers(0, len(absent), 2000)]
    probe += [build[i] for i in r.integers(0, n, 4000)]
    return build, [probe[i] for i in r.permutation(8000)], held, off


@pytest.mark.gpu
def test_utf8_key_group_by_join_and_semi_through_dictionary_clusters(gpu):
    """utf8_codes_build_kernel / utf8_codes_probe_kernel: GROUP BY a text column (dense accumulators and hashed ones), an inner join and a semi /
    anti join on it.  A probe string that differs from a build string in its last byte alone, in the same run of slots, must stay absent."""
    r = np.random.default_rng(1613)
    build, probe, held, off = _utf8_sides()
    assert any(a[:-1] == b[:-1] for a in held for b in off) or any(a != b and a[:-1] == b[:-1] for a in held for b in held)
    t = {"s": build, "v": [int(x) for x in r.integers(-10**6, 10**6, 6000)], "f": [None if x < 0.2 else float(int(x * 100)) for x in r.random(6000)]}
    right = {"s_r": probe, "y": list(range(8000))}
    for aggs in (AGG3, [("count", "f", "UInt64"), ("min", "f", "Float64")]):
        want = _srt(K._oracle_rows(t, ["s"], aggs))
        for chunk in (None, CHUNK):
            got, ran = _run(gpu, K._group_plan(["s"], aggs, UCOLS), [(t, UCOLS)], chunk)
            assert "utf8_codes_build_kernel" in ran and "key_codes_insert_kernel" not in ran, sorted(ran)
            assert _srt(got) == want, (aggs, chunk, len(got), len(want))
    want = _srt(g.rows(g.hash_join_inner(t, right, [("s", "s_r")])))
    for chunk in (None, CHUNK):
        got, ran = _run(gpu, K._join_plan(UCOLS, URCOLS, [("s", "s_r")]), [(t, UCOLS), (right, URCOLS)], chunk)
        assert "utf8_codes_build_kernel" in ran and "utf8_codes_probe_kernel" in ran, sorted(ran)
        assert _srt(got) == want and len(want) > 8000, (chunk, len(got), len(want))
    for jt in ("Semi", "Anti"):
        plan = S._semi_plan(jt, [("s_r", "s")], lcols=URCOLS, rcols=UCOLS)
        want = table_rows(semi_anti_table(right, t, [("s_r", "s")], jt == "Anti"), ["s_r", "y"])
        for chunk in (None, CHUNK):
            got, ran = _run(gpu, plan, [(right, URCOLS), (t, UCOLS)], chunk)
            assert "utf8_codes_build_kernel" in ran and "utf8_codes_probe_kernel" in ran, sorted(ran)
            assert got == want and 1500 < len(want) < 6500, (jt, chunk, len(got), len(want))


@pytest.mark.gpu
def test_distinct_int32_utf8_through_searched_pair_clusters(gpu):
    """relops.hip distinct_insert_kernel, keys NOT increasing (the hash set, not the ordered shortcut): four clusters of 32 (key, text) pairs found by
    search for a table of exactly 16384 slots, every pair several times, among 1500 ordinary pairs."""
    r = np.random.default_rng(1614)
    n = 6000
    pairs = [p for c in hc.search_pairs(hc.pow2_at_least(2 * n), 32, count=4) for p in c]
    pairs += [(int(k), "n%d" % x) for k, x in zip(r.integers(-2**31, 2**31, 1500), r.integers(0, 48, 1500))]
    rows = pairs * 2
    rows += [pairs[i] for i in r.integers(0, len(pairs), n - len(rows))]
    rows = [rows[i] for i in r.permutation(n)]
    cols = [("j", "Int32"), ("s", "Utf8")]
    t = {"j": [k for k, _ in rows], "s": [s for _, s in rows]}
    assert any(a >= b for a, b in zip(t["j"], t["j"][1:]))
    for chunk in (None, CHUNK):
        got, ran = _run(gpu, K._group_plan(["j", "s"], [], cols), [(t, cols)], chunk)
        assert "distinct_insert_kernel" in ran and "key_codes_insert_kernel" not in ran, sorted(ran)
        assert sorted(got) == sorted(set(pairs)), (chunk, len(got), len(set(pairs)))


# ------------------------------------------------------------------ (i) the cut-offs
def _ordinary_plan_still_runs(gpu):
    """after a refused call: the same GpuContext groups ordinary rows correctly"""
    t = {"k": [i % 97 * 10**10 for i in range(3000)], "x": [i % 5 for i in range(3000)], "f": [float(i % 13) for i in range(3000)], "v": list(range(3000))}
    got, _ = _run(gpu, K._group_plan(["k"], GAGG, GCOLS), [(t, GCOLS)])
    assert _srt(got) == _srt(K._oracle_rows(t, ["k"], GAGG)) and len(got) == 97


@pytest.mark.gpu
def test_count_distinct_at_and_beyond_its_probe_limit(gpu):
    """distinct.hip cuts a probe off after kMaxProbe = 2048 slots.  Why the call is bounded (distinct_count_by_group's pass loop): a pass whose
    insert kernel reports a cut probe is repeated ONCE with `full` = pow2_at_least(2 * rows) slots if it ran on a smaller, hint-sized table
    (`cap = full`), and a pass that ran at `full` ends the call with FLOCKGPU_ERR_CAPACITY (`if (cap >= full) return fail(...)`): at most two
    passes, each row at most 2048 probes, nothing written for a cut row.  A fresh context has no hint: one pass.
    2048 values of ONE home slot fit exactly (the last one is found on probe 2047); with 2049 the call must fail, never return a number."""
    from flock_amd import FlockGpuError, _ffi
    for count in (2048, 2049):
        values = hc.home_cluster(0xFFFFFF, count)
        t, rows = _dc_table(values, count)
        t["l"] = rows
        if count == 2048:
            for chunk in (None, CHUNK):
                got, want, ran = _dc(gpu, t, [], "l", chunk=chunk)
                assert "distinct_insert_kernel" in ran and got == want == [(2048,)], (chunk, got)
        else:
            with pytest.raises(FlockGpuError) as e:
                _dc(gpu, t, [], "l")
            assert e.value.code == _ffi.ERR_CAPACITY and "distinct table overflow" in str(e.value), str(e.value)
            _ordinary_plan_still_runs(gpu)


@pytest.mark.gpu
def test_group_by_at_and_beyond_its_probe_limit(gpu):
    """claim_slot cuts a probe off after kClaimProbes = 4096 slots.  Why the call is bounded (group_by_key64_n's pass loop): the insert kernel sets
    the error word, every wave leaves its loop at its next step, and the host repeats the pass ONCE at `full` = pow2_at_least(2 * rows) slots if
    the table was hint-sized (`cap = full`), else returns FLOCKGPU_ERR_CAPACITY (`if (cap >= full) return fail(...)`): at most two passes.
    4096 keys of ONE home slot are grouped exactly; with 4097 the call must fail with "group table overflow"."""
    from flock_amd import FlockGpuError, _ffi
    for count in (4096, 4097):
        r = np.random.default_rng(count)
        keys = hc.home_cluster(0xFFFFFF, count)
        rows = keys * 2
        rows = [rows[i] for i in r.permutation(len(rows))]
        n = len(rows)
        t = {"k": rows, "x": [None if i % 3 == 0 else i for i in range(n)], "f": [float(i % 1000) for i in range(n)], "v": [0] * n}
        plan = K._group_plan(["k"], GAGG, GCOLS)
        if count == 4096:
            want = _srt(K._oracle_rows(t, ["k"], GAGG))
            for chunk in (None, CHUNK):
                got, ran = _run(gpu, plan, [(t, GCOLS)], chunk)
                assert "group_insert_n_kernel" in ran and _srt(got) == want and len(got) == 4096, (chunk, len(got))
        else:
            with pytest.raises(FlockGpuError) as e:
                _run(gpu, plan, [(t, GCOLS)])
            assert e.value.code == _ffi.ERR_CAPACITY and "group table overflow" in str(e.value), str(e.value)
            _ordinary_plan_still_runs(gpu)


@pytest.mark.gpu
def test_a_run_of_3000_slots_in_the_tables_without_a_cut_off(gpu):
    """The join table, the semi join's key set, key_codes and the Utf8 dictionary probe until they find their key or a free slot.  3000 of 6000 build
    rows in ONE run of occupied slots (integer keys and steered tuples: one home; strings, which cannot be steered: two per slot over 1500
    neighbouring slots): the exact result."""
    r = np.random.default_rng(1616)
    n = 6000
    run = hc.home_cluster(0x3FFFF0, 3000)                       # (16 slots before the end of a 16384-slot table: the run wraps)
    other = [int(x) for x in r.integers(-2**62, 2**62, 3000)]
    order = r.permutation(n)
    build = [(run + other)[i] for i in order]
    absent = hc.home_cluster(0x3FFFF0, 200, first=3000) + hc.behind(0x3FFFF0, 2999, 100)
    probe = [(build + absent)[i] for i in r.integers(0, n + 300, 9000)]
    lcols, rcols = _jcols("Int64", "Int64")
    left, right = _join_tables(build, probe, 6)
    got, ran = _run(gpu, K._join_plan(lcols, rcols, [("a", "b")]), [(left, lcols), (right, rcols)], CHUNK)
    assert "join_hash_build_kernel" in ran, sorted(ran)
    assert _srt(got) == _srt(g.rows(g.hash_join_inner(left, right, [("a", "b")]))) and len(got) > 8000
    sleft, sright = {"a": probe, "x": [0] * 9000}, {"b": build, "y": list(range(n))}
    for jt in ("Semi", "Anti"):
        _semi_check(gpu, jt, sleft, sright, SLCOLS, SRCOLS, ["semi_set_build_kernel", "semi_probe_set_flag_kernel"], ["semi_tiny_kernel"])
    # key_codes: 3000 tuples steered to one home (their tags differ), GROUP BY and a join's probe
    firsts = [None if m % 9 == 4 else m % 5 for m in range(n)]
    target = lambda m: (hc._tag_of(m) << 32) | ((m & 0xFF) << 24) | 0x3FFFF0
    seconds = [hc.steer_last_i64(hc.prefix_hash([firsts[m]]), target(m)) if m < 3000 else other[m - 3000] for m in range(n)]
    t = {"a": [firsts[i] for i in order], "b": [seconds[i] for i in order], "s": [""] * n, "bs": [0] * n, "v": list(range(n)), "f": [1.0] * n}
    got, ran = _run(gpu, K._group_plan(["a", "b"], AGG3, ACOLS), [(t, ACOLS)], CHUNK)
    assert "key_codes_insert_kernel" in ran and got == K._oracle_rows(t, ["a", "b"], AGG3) and len(got) == n
    pr = {"a_r": [t["a"][i] for i in range(0, n, 2)] + [1] * 500, "b_r": [t["b"][i] for i in range(0, n, 2)] + [hc.steer_last_i64(hc.prefix_hash([1]), target(m)) for m in range(500)],
          "s_r": [""] * 3500, "bs_r": [0] * 3500, "p": list(range(3500))}
    on = [("a", "a_r"), ("b", "b_r")]
    got, ran = _run(gpu, K._join_plan(ACOLS, PCOLS, on), [(t, ACOLS), (pr, PCOLS)], CHUNK)
    assert "key_codes_probe_kernel" in ran and _srt(got) == _srt(g.rows(g.hash_join_inner(t, pr, on))) and len(got) > 2000
    # the Utf8 dictionary
    texts = hc.search_utf8_run(hc.pow2_at_least(2 * n), 1500, 2)
    strings = texts + ["u%d" % x for x in r.integers(0, 10**9, 3000)]
    ut = {"s": [strings[i] for i in order], "v": list(range(n)), "f": [1.0] * n}
    got, ran = _run(gpu, K._group_plan(["s"], AGG3, UCOLS), [(ut, UCOLS)], CHUNK)
    assert "utf8_codes_build_kernel" in ran and _srt(got) == _srt(K._oracle_rows(ut, ["s"], AGG3)) and len(got) == len(set(strings))
