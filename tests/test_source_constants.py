"""Constants that a GPU test restates in Python must be the kernels' own (CPU: reads the sources, no GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(name):
    with open(os.path.join(ROOT, "flock_amd", "csrc", name)) as f:
        return f.read()


def test_q8_bucket_sizing_in_the_parity_test_is_the_kernels():
    """tests/test_gpu_parity.py::_q8_part_log2 / _q8_part_bucket build inputs that land in ONE hash bucket of q8's grouped hash path:
    they must size and hash exactly as q8.hip does."""
    q8, tab = _src("q8.hip"), _src("hashtab.hpp")
    m = re.search(r"kPartPersonsPerBucket = (\d+), kPartAuctionsPerBucket = (\d+);", q8)
    assert m, "q8.hip no longer states the bucket sizing in the form the test reads"
    persons, auctions = int(m.group(1)), int(m.group(2))
    max_log2 = int(re.search(r"constexpr int kPartMaxLog2 = (\d+);", q8).group(1))
    fib = int(re.search(r"constexpr uint32_t kFibHash = (0x[0-9A-Fa-f]+)u;", tab).group(1), 16)
    with open(os.path.join(ROOT, "tests", "test_gpu_parity.py")) as f:
        test = f.read()
    assert f"while l < {max_log2} and ((max_p >> l) > {persons} or (max_a >> l) > {auctions}):" in test
    assert f"np.uint32(0x{fib:08X})" in test
    assert "return log2nb ? (k * kFibHash) >> (32 - log2nb) : 0u;" in q8          # the bucket = the hash's top bits


# ------------------------------------------------------------------ tests/hash_craft.py restates the operators' hashes: each mirror against the kernel text
def _hex(v):
    return "0x%Xull" % v


def test_mix64_in_relops_and_distinct_is_hash_crafts():
    """tests/hash_craft.py inverts mix64 to make keys that share a tag and a home slot: both copies of the finaliser must be the mirrored one."""
    import hash_craft as hc
    lines = ["x ^= x >> 30; x *= %s;" % _hex(hc.MIX_A), "x ^= x >> 27; x *= %s;" % _hex(hc.MIX_B), "return x ^ (x >> 31);"]
    for name in ("relops.hip", "distinct.hip"):
        src = _src(name)
        at = src.index("__device__ __forceinline__ uint64_t mix64(uint64_t x) {")
        body = [ln.strip() for ln in src[at:].splitlines()[1:4]]
        assert body == lines, (name, body)


def test_key_tuple_hash_and_hash_bytes_are_hash_crafts():
    import hash_craft as hc
    src = _src("relops.hip")
    at = src.index("__device__ __forceinline__ uint64_t key_tuple_hash(const KeyTuple &k, int64_t i, bool *any_null) {")
    body = src[at:src.index("// row a of tuple ka equals row b of tuple kb")]
    assert "uint64_t h = %s;" % _hex(hc.TUPLE_SEED) in body                                  # the seed
    assert "v = %s * (uint64_t)(c + 1);" % _hex(hc.NULL_MARK) in body                        # a NULL: the marker of its column number
    assert "h = mix64((h * %s) ^ v);" % _hex(hc.FNV_PRIME) in body                           # the step: the LAST column steers the hash
    assert "v = (uint64_t)load_as_i64(k.values[c], k.type[c], i);" in body                   # integers widened (Int32 with its sign)
    assert "v = hash_bytes(static_cast<const uint8_t *>(k.values[c]) + off[i], off[i + 1] - off[i]);" in body
    assert "(int64_t) static_cast<const int32_t *>(v)[i]" in src[src.index("int64_t load_as_i64("):][:300]
    at = src.index("__device__ __forceinline__ uint64_t hash_bytes(const uint8_t *p, int32_t len) {")
    body = [ln.strip() for ln in src[at:].splitlines()[1:4]]
    assert body == ["uint64_t h = %s;" % _hex(hc.FNV_BASIS), "for (int32_t b = 0; b < len; ++b) h = (h ^ p[b]) * %s;" % _hex(hc.FNV_PRIME),
                    "return mix64(h ^ (uint64_t)(uint32_t)len);"], body
    # the slots hold {hash >> 32, first row}; the home is the hash's low bits
    for kernel in ("void key_codes_insert_kernel(", "void key_codes_probe_kernel("):
        body = src[src.index(kernel):][:1500]
        assert "tag = h >> 32" in body and "uint64_t s = h & (cap - 1);" in body and "s = (s + 1) & (cap - 1);" in body, kernel
    # the dictionaries of one Utf8 column
    for kernel in ("void utf8_codes_build_kernel(", "void utf8_codes_probe_kernel("):
        assert "uint64_t s = hash_bytes(me, len) & (cap - 1);" in src[src.index(kernel):][:900], kernel


def test_the_distinct_hashes_are_hash_crafts():
    import hash_craft as hc
    d = _src("distinct.hip")
    assert "const uint64_t h = mix64(v + (uint64_t)(uint32_t)g * %s);" % _hex(hc.PAIR_STEP) in d          # same_hash_pairs
    assert "const uint64_t tag = h >> 32, mine = (tag << 32) | (uint32_t)i;" in d and "uint64_t s = h & (cap - 1);" in d
    assert "if (kI32) return (uint64_t)(int64_t) static_cast<const int32_t *>(v)[i];" in d                 # an Int32 argument hashes sign-extended
    r = _src("relops.hip")
    body = r[r.index("__global__ __launch_bounds__(kBlock) void distinct_insert_kernel("):][:1400]         # DISTINCT (Int32, Utf8)
    assert "uint64_t h = %s ^ (uint64_t)(uint32_t)key[i];" % _hex(hc.FNV_BASIS) in body
    assert "for (int32_t b = off[i]; b < off[i + 1]; ++b) h = (h ^ bytes[b]) * %s;" % _hex(hc.FNV_PRIME) in body
    assert "uint64_t s = mix64(h) & (cap - 1);" in body


def test_the_integer_tables_hash_mix64_of_the_key():
    """claim_slot, the LDS group table, the join build and lookup, the key set and the two one-workgroup kernels: home = mix64(key) & (slots - 1)."""
    r = _src("relops.hip")
    assert r.count("mix64((uint64_t)key) & (cap - 1)") == 4                       # claim_slot, join build, join_hash_home, semi_set_build
    assert "uint64_t join_hash_home(uint64_t cap, int64_t key) { return key == kEmptyKey ? cap : mix64((uint64_t)key) & (cap - 1); }" in r
    assert r.count("(uint32_t)mix64((uint64_t)key) & (kTinySlots - 1)") == 4      # join_tiny build + probe, semi_tiny build + probe
    assert "uint32_t s = (uint32_t)mix64((uint64_t)key) & (lds_slots - 1);" in r
    assert "const uint32_t lds_slots = width <= 2 ? 2048u : 1024u;" in r and "const int64_t rows_per_wg = (int64_t)lds_slots * 4;" in r
    assert "if (rows >= rows_per_wg * 4 && sp.n > 0) {" in r                      # tests/test_plan_hash_collisions.py LDS_SWITCH
    assert "constexpr int kCombineMin = 8;" in r


def test_slot_of_and_the_probe_limits_are_hash_crafts():
    import hash_craft as hc
    tab, r = _src("hashtab.hpp"), _src("relops.hip")
    assert "constexpr uint32_t kFibHash = 0x%Xu;" % hc.FIB in tab
    assert "return (uint32_t)(((uint64_t)(key * kFibHash) * cap) >> 32);" in tab
    assert "constexpr uint32_t kMaxProbe = 2048;" in tab                          # distinct.hip's cut-off
    assert "const uint32_t limit = cap < (uint64_t)kMaxProbe ? (uint32_t)cap : kMaxProbe;" in _src("distinct.hip")
    assert "constexpr uint64_t kClaimProbes = 4096;" in r
    assert "for (uint64_t probe = 0, lim = cap < kClaimProbes ? cap : kClaimProbes; probe < lim; ++probe) {" in r
    assert "constexpr int kLdsGroupProbes = 8;" in r and "for (int probe = 0; probe < kLdsGroupProbes; ++probe) {" in r
    assert "constexpr int kTinyBuild = 4096, kTinySlots = 8192, kTinyThreads = 1024, kTinyProbe = 1 << 16;" in r
    assert "bool semi_is_tiny(int64_t n_left, int64_t n_right) { return n_left > 0 && n_right > 0 && n_right <= kTinyBuild && n_left <= kTinyProbe; }" in r
    assert "return n_left > 0 && n_right > 0 && std::min(n_left, n_right) <= kTinyBuild && std::max(n_left, n_right) <= kTinyProbe;" in r


def test_every_table_is_sized_pow2_at_least_twice_its_rows():
    """The GPU tests search Int32 and Utf8 clusters at the exact table size: every operator must size as hash_craft.pow2_at_least(2 * rows) does."""
    import hash_craft as hc
    r, d = _src("relops.hip"), _src("distinct.hip")
    for src in (r, d):
        at = src.index("uint64_t pow2_at_least(uint64_t v) {")
        assert [ln.strip() for ln in src[at:].splitlines()[1:4]] == ["uint64_t c = 1024;", "while (c < v) c <<= 1;", "return c;"]
    assert hc.pow2_at_least(0) == 1024
    size = "pow2_at_least((uint64_t)std::max<int64_t>(%s, 1) * 2);"
    hinted = "uint64_t cap = hint.empty() || hint[0] <= 0 ? full : std::min(full, pow2_at_least((uint64_t)std::max<int64_t>((hint[0] - 1) * 3, 1024)));"

    def body(src, head):
        return src[src.index(head):][:9000]
    for head, rows in (("int distinct_i32_utf8(", "rows"), ("int utf8_codes(", "n_build"), ("int key_codes(", "rows"), ("int join_hashed(", "n_left"),
                       ("int semi_rows(", "n_right")):
        assert "const uint64_t cap = " + size % rows in body(r, head), head
    for src, head in ((r, "int group_by_key64_n("), (d, "int distinct_count_by_group(")):
        b = body(src, head)
        assert "const uint64_t full = " + size % "rows" in b and hinted in b, head
        # the pass loop: a hint-sized table that overflows is tried ONCE more at `full`, a full-sized one that overflows is an error
        assert "if (cap >= full) return fail(ctx, FLOCKGPU_ERR_CAPACITY," in b and "cap = full;" in b, head
    assert '"%s: group table overflow"' in r and '"%s: distinct table overflow"' in d


def test_the_fused_paths_size_and_hash_as_the_collision_tests_assume():
    """tests/test_gpu_fused_hash_collisions.py: fib_cluster ids share a home in every hashtab.hpp table, q8's bucket and the slots inside it are the top
    bits of key * kFibHash, q13 probes from LDS up to kLdsSlots slots of 2 * rows + 1, q3 builds in LDS up to kLdsBuildCap slots of 1.5 per person;
    the packed (Int32, Int32) GROUP BY key of tests/test_plan_hash_collisions.py is first column high, second low."""
    q3, q8, q13, r = _src("q3.hip"), _src("q8.hip"), _src("q13.hip"), _src("relops.hip")
    assert "out[i] = (int64_t)(((uint64_t)(uint32_t)a[i] << 32) | (uint64_t)(uint32_t)b[i]);" in r
    assert "uint32_t part_bucket(uint32_t k, int log2nb) { return log2nb ? (k * kFibHash) >> (32 - log2nb) : 0u; }" in q8
    assert "return ((k * kFibHash) >> (32 - log2nb - log2slots)) & ((1u << log2slots) - 1u);" in q8
    assert "constexpr int kJoinSlotsLog2 = 10, kJoinSlots = 1 << kJoinSlotsLog2;" in q8 and "constexpr int kJoinSellLog2 = 12, kJoinSellLog2Large = 14;" in q8
    assert "constexpr int kJoinProbes = 128;" in q8                               # the clusters of 64 stay below it
    assert "constexpr int kLdsSlots = 16384;" in q13 and "const bool lds = cap <= (uint32_t)kLdsSlots;" in q13
    assert "uint32_t cap = (uint32_t)std::max<int64_t>(64, side_rows * 2 + 1);" in q13
    assert q13.count("uint32_t s = slot_of((uint32_t)key, cap);") == 2          # find_global, find_lds
    assert "constexpr uint32_t kLdsBuildCap = 18432;" in q3
    assert "const uint64_t cap64 = std::max<uint64_t>(64, (uint64_t)max_person_rows * 3 / 2 + 8);" in q3
    assert q3.count("slot_of((uint32_t)sv[") == 2                                 # the probes of the global tables and of the LDS build


def test_the_json_edge_tests_restate_json_hips_constants_and_messages():
    """tests/test_gpu_json_edges.py crafts bytes onto the seams of the line index and of the stage, and tests/json_ref.py words the errors: the tile,
    the lines per workgroup, the stage, the formula that sizes it, the depth bound and the seven messages must be json.hip's own."""
    import json_ref
    j, scan = _src("json.hip"), _src("scan.hpp")
    with open(os.path.join(ROOT, "tests", "test_gpu_json_edges.py")) as f:
        test = f.read()
    assert "constexpr int kBlock = 256;" in scan
    assert "constexpr int kNlBytes = 64;" in j and "constexpr int kNlTile = kBlock * kNlBytes;" in j and "TILE = 256 * 64 " in test
    assert "constexpr int kParseLines = kBlock;" in j and "LINES = 256 " in test
    assert "constexpr int kStageBytes = 48 * 1024;" in j and "STAGE_MAX = 48 * 1024 " in test
    assert "const int64_t want = (n_bytes / std::max<int64_t>(n_lines, 1) + 1) * kParseLines * 5 / 4 + 64;" in j
    assert "want = (n_bytes // max(n_lines, 1) + 1) * LINES * 5 // 4 + 64" in test
    assert "const int32_t stage_bytes = (int32_t)std::min<int64_t>(kStageBytes, (want + 1023) & ~int64_t(1023));" in j
    assert "return min(STAGE_MAX, (want + 1023) & ~1023)" in test
    assert "const int32_t a0 = b0 & ~15;" in j and "const bool staged = b1 - a0 + 16 <= stage_bytes;" in j
    assert "return b1 - (b0 & ~15) + 16, stage_bytes(len(text), n_lines)" in test and "return span <= stage" in test
    assert "constexpr int kMaxDepth = %d;" % json_ref.MAX_DEPTH in j
    m = re.search(r"enum : uint32_t \{ kErrSyntax = 1, kErrNumber = 2, kErrMissing = 3, kErrBlank = 4, kErrKeyEscape = 5, kErrRange = 6, kErrDepth = 7 \};", j)
    assert m, "json.hip's error codes are no longer the seven of tests/json_ref.py"
    table = j[j.index("static const char *what[] = {"):]
    table = table[:table.index("};")]
    assert re.findall(r'"([^"]*)"', table) == [""] + [json_ref.MESSAGES[c] for c in ("malformed", "number", "missing", "blank", "key_escape", "range", "depth")]
    status = j[j.index("return fail(ctx, code == kErrNumber"):][:200]
    assert "code == kErrNumber || code == kErrBlank || code == kErrKeyEscape || code == kErrDepth ? FLOCKGPU_ERR_UNSUPPORTED : FLOCKGPU_ERR_INVALID" in status
    assert sorted(c for c, s in json_ref.STATUS.items() if s == "unsupported") == ["blank", "depth", "key_escape", "number"]
