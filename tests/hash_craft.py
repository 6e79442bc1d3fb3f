"""Crafted hash collisions for the operators' open-addressing tables (plain Python / numpy, no GPU).

The kernels' hashes are restated here once (tests/test_source_constants.py pins every one of them to the kernel text), and because they are
invertible, inputs that random data never produces are cheap to make:

  * relops.hip / distinct.hip `mix64` is the splitmix64 finaliser, a bijection: `mix64_inv((tag << 32) | (m << 24) | low24)` for m = 0..255 are
    256 different Int64 keys with ONE 32-bit tag and ONE home slot in every power-of-two table of up to 2^24 slots;
  * `key_tuple_hash` ends in `mix64((h * 0x100000001B3) ^ v)`: the last Int64 column of a tuple steers the whole hash, whatever stands before it;
  * distinct.hip hashes `mix64(v + gid * 0x9E3779B97F4A7C15)`: the pairs (g, X - g * 0x9E3779B97F4A7C15) have IDENTICAL 64-bit hashes;
  * hashtab.hpp `slot_of` is `(key * kFibHash * cap) >> 32` with an odd multiplier: the keys ((T << 12 | j) * kFibHash^-1) mod 2^32 share a home in
    every table of up to 2^20 slots;
  * Int32 keys and Utf8 bytes cannot be steered: their home-slot clusters are found by search at the exact table size (`search_*`).

tests/test_hash_craft.py decides whether these inputs are what they claim."""
import numpy as np

M64 = (1 << 64) - 1
MIX_A, MIX_B = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MIX_A_INV, MIX_B_INV = 0x96DE1B173F119089, 0x319642B2D24D8EC3          # the multipliers' inverses modulo 2^64
FNV_BASIS, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3
TUPLE_SEED, NULL_MARK = 0x9E3779B97F4A7C15, 0x6A09E667F3BCC909
PAIR_STEP = 0x9E3779B97F4A7C15
FIB = 0x9E3779B1
FIB_INV = pow(FIB, -1, 1 << 32)
INT64_MIN = -(1 << 63)


# ------------------------------------------------------------------ mirrors of the kernels' hashes
def mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * MIX_A) & M64
    x ^= x >> 27
    x = (x * MIX_B) & M64
    return x ^ (x >> 31)


def mix64_inv(x):
    x &= M64
    x ^= (x >> 31) ^ (x >> 62)
    x = (x * MIX_B_INV) & M64
    x ^= (x >> 27) ^ (x >> 54)
    x = (x * MIX_A_INV) & M64
    return x ^ (x >> 30) ^ (x >> 60)


def mix64_np(x):
    """mix64 over a uint64 array (numpy's unsigned multiplication wraps)"""
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(MIX_A)
    x ^= x >> np.uint64(27)
    x *= np.uint64(MIX_B)
    return x ^ (x >> np.uint64(31))


def signed(x):
    """the 64-bit pattern x as an Int64 value"""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def _as_bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def hash_bytes(s):
    """relops.hip hash_bytes: FNV-1a over the bytes, then mix64(h ^ len)"""
    b = _as_bytes(s)
    h = FNV_BASIS
    for c in b:
        h = ((h ^ c) * FNV_PRIME) & M64
    return mix64(h ^ len(b))


def tuple_step(h, v):
    return mix64(((h * FNV_PRIME) & M64) ^ (v & M64))


def key_tuple_hash(values):
    """relops.hip key_tuple_hash of one row: values = the row's key columns in order -- None (NULL: the marker of its column number), an integer
    (Int32 / Int64 / UInt64 / Timestamp: widened to 64 bits, an Int32 sign-extended) or str / bytes (Utf8: hash_bytes)."""
    h = TUPLE_SEED
    for c, v in enumerate(values):
        if v is None:
            v = (NULL_MARK * (c + 1)) & M64
        elif isinstance(v, (str, bytes)):
            v = hash_bytes(v)
        h = tuple_step(h, v)
    return h


def distinct_pair_hash(gid, value):
    """distinct.hip: the hash of (group id, argument bits -- an Int32 argument sign-extended)"""
    return mix64((value + (gid & 0xFFFFFFFF) * PAIR_STEP) & M64)


def distinct_i32_utf8_hash(key, text):
    """relops.hip distinct_insert_kernel, DISTINCT (Int32, Utf8)"""
    h = FNV_BASIS ^ (key & 0xFFFFFFFF)
    for c in _as_bytes(text):
        h = ((h ^ c) * FNV_PRIME) & M64
    return mix64(h)


def slot_of(key, cap):
    """hashtab.hpp slot_of: cap need not be a power of two"""
    return ((((key & 0xFFFFFFFF) * FIB) & 0xFFFFFFFF) * cap) >> 32


def pow2_at_least(v):
    c = 1024
    while c < v:
        c <<= 1
    return c


def home(h, cap):
    return h & (cap - 1)


# ------------------------------------------------------------------ makers
def _tag_of(i):
    """different tags for different i < 2^32 (an odd multiplier: a bijection of the 32-bit words)"""
    return ((i + 1) * 0x9E3779B1) & 0xFFFFFFFF


def tag_cluster(tag, low24, n):
    """n <= 256 Int64 keys whose mix64 has the 32-bit tag `tag` and the low 24 bits `low24`: one tag, one home in every table of up to 2^24 slots"""
    assert 0 <= n <= 256 and 0 <= tag <= 0xFFFFFFFF and 0 <= low24 <= 0xFFFFFF
    keys = [signed(mix64_inv((tag << 32) | (m << 24) | low24)) for m in range(n)]
    assert INT64_MIN not in keys
    return keys


def home_cluster(low24, n, first=0):
    """n Int64 keys of pairwise different tags whose mix64 has the low 24 bits `low24`; `first` numbers the tags (two calls with disjoint ranges of
    first .. first + n give disjoint keys)"""
    assert 0 <= low24 <= 0xFFFFFF and first + n < (1 << 32)
    keys = [signed(mix64_inv((_tag_of(first + i) << 32) | (((first + i) & 0xFF) << 24) | low24)) for i in range(n)]
    assert INT64_MIN not in keys
    return keys


def behind(low24, distance, n, first=1 << 20):
    """n keys whose home lies `distance` slots behind that of a cluster at low24 (wrapping with the table): their probes walk through the cluster"""
    return home_cluster((low24 + distance) & 0xFFFFFF, n, first)


def prefix_hash(values):
    """key_tuple_hash's state after the columns `values`: what steer_last_i64 takes"""
    return key_tuple_hash(values)


def steer_last_i64(prefix, target):
    """the Int64 value of a tuple's LAST column that makes the tuple's hash `target`, given the hash state `prefix` of the columns before it"""
    return signed(mix64_inv(target) ^ ((prefix * FNV_PRIME) & M64))


def same_hash_pairs(x, groups):
    """[(g, value)]: for every group id g the Int64 value whose (g, value) pair hashes exactly as (0, x) does"""
    return [(g, signed(x - (g & 0xFFFFFFFF) * PAIR_STEP)) for g in groups]


def fib_cluster(top20, n):
    """n <= 4096 uint32 keys whose slot_of is the same in every table of up to 2^20 slots (key * kFibHash = top20 << 12 | j)"""
    assert 0 <= n <= 4096 and 0 <= top20 < (1 << 20)
    return [(((top20 << 12) | j) * FIB_INV) & 0xFFFFFFFF for j in range(n)]


def _fullest(homes, n, count, ok=None):
    """the `count` fullest buckets of `homes` (an array of slot numbers) with at least n members each: lists of candidate indices"""
    order = np.argsort(homes, kind="stable")
    sh = homes[order]
    starts = np.flatnonzero(np.r_[True, sh[1:] != sh[:-1]])
    sizes = np.diff(np.r_[starts, len(sh)])
    out = []
    for b in np.argsort(-sizes, kind="stable"):
        if sizes[b] < n:
            break
        members = order[starts[b]:starts[b] + sizes[b]]
        if ok is None or ok(members):
            out.append(members)
            if len(out) == count:
                break
    assert len(out) == count, "the search found %d of %d clusters of %d" % (len(out), count, n)
    return out


I32_CANDIDATES = np.arange(-(1 << 20), 1 << 20, dtype=np.int64) * 2039          # 2^21 values over the whole Int32 range


def search_i32(cap, n, count=1):
    """`count` clusters of n Int32 values each that share a home slot in a table of exactly `cap` slots (mix64 of the sign-extended value)"""
    homes = (mix64_np(I32_CANDIDATES.astype(np.uint64)) & np.uint64(cap - 1)).astype(np.int64)
    return [[int(v) for v in I32_CANDIDATES[m[:n]]] for m in _fullest(homes, n, count)]


def _fnv_np(h, texts):
    """FNV-1a steps over equally many strings, grouped by length; h: uint64 start values -> uint64"""
    h = h.copy()
    lens = np.array([len(t) for t in texts])
    for ln in np.unique(lens):
        idx = np.flatnonzero(lens == ln)
        mat = np.frombuffer(b"".join(texts[i] for i in idx), dtype=np.uint8).reshape(len(idx), ln) if ln else np.zeros((len(idx), 0), np.uint8)
        x = h[idx]
        for k in range(ln):
            x = (x ^ mat[:, k].astype(np.uint64)) * np.uint64(FNV_PRIME)
        h[idx] = x
    return h, lens


UTF8_CANDIDATES = [b"s%d" % i for i in range(400_000)]


def utf8_homes(cap, texts=UTF8_CANDIDATES):
    h, lens = _fnv_np(np.full(len(texts), FNV_BASIS, np.uint64), texts)
    return (mix64_np(h ^ lens.astype(np.uint64)) & np.uint64(cap - 1)).astype(np.int64)


def search_utf8(cap, n, count=1):
    """`count` clusters of at least n strings each that share a home slot in a Utf8 dictionary of exactly `cap` slots.  Every cluster holds two
    strings that differ only in their last byte, and strings of different lengths."""
    texts = UTF8_CANDIDATES
    number = {t: i for i, t in enumerate(texts)}

    def ok(members):
        ms = set(int(i) for i in members)
        if len({len(texts[i]) for i in ms}) < 2:
            return False
        for i in ms:
            t = texts[i]
            for d in b"0123456789":
                j = number.get(t[:-1] + bytes([d]))
                if j is not None and j != i and j in ms:
                    return True
        return False
    return [[texts[i].decode() for i in m] for m in _fullest(utf8_homes(cap, texts), n, count, ok)]


def search_utf8_run(cap, slots, per_slot, start=None):
    """per_slot strings for each of `slots` neighbouring home slots (from `start`, wrapping; default: half the run before the table's end) of a Utf8
    dictionary of exactly `cap` slots: slots * per_slot strings that fill ONE run of occupied slots at least that long"""
    start = cap - slots // 2 if start is None else start
    homes = utf8_homes(cap)
    order = np.argsort(homes, kind="stable")
    first = np.searchsorted(homes[order], np.arange(cap + 1))
    out = []
    for k in range(slots):
        s = (start + k) & (cap - 1)
        assert first[s + 1] - first[s] >= per_slot, "slot %d has fewer than %d candidates" % (s, per_slot)
        out += [UTF8_CANDIDATES[i].decode() for i in order[first[s]:first[s] + per_slot]]
    return out


PAIR_TEXTS = [b"n%d" % i for i in range(48)]
PAIR_KEYS = (np.arange(8192, dtype=np.int64) - 4096) * 7919


def search_pairs(cap, n, count=1):
    """`count` clusters of n (Int32 key, text) pairs each that share a home slot in DISTINCT (Int32, Utf8)'s table of exactly `cap` slots"""
    keys = np.tile(PAIR_KEYS, len(PAIR_TEXTS))
    texts = [t for t in PAIR_TEXTS for _ in range(len(PAIR_KEYS))]
    h, _ = _fnv_np(np.uint64(FNV_BASIS) ^ (keys.astype(np.uint64) & np.uint64(0xFFFFFFFF)), texts)
    homes = (mix64_np(h) & np.uint64(cap - 1)).astype(np.int64)
    return [[(int(keys[i]), texts[i].decode()) for i in m[:n]] for m in _fullest(homes, n, count)]
