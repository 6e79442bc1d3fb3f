"""tests/hash_craft.py makes what it claims (CPU): the inverses invert, every maker's output collides under the mirrors of the kernels' hashes to the
stated bit counts and cluster sizes, and the keys inside a cluster are pairwise different.  The GPU tests take the crafted inputs on this file's word."""
import numpy as np
import pytest

import hash_craft as hc

TAGS = [0, 0xFFFFFFFF, 0x12345678]
LOWS = [0, 0xFFFFFF, 0x00ABCD]
CAPS = [1024, 8192, 16384, 1 << 20, 1 << 24]


def test_mix64_and_its_inverse_round_trip():
    r = np.random.default_rng(64)
    xs = [0, 1, hc.M64, 1 << 63, 0x9E3779B97F4A7C15] + [int(v) for v in r.integers(0, 1 << 64, 100_000, dtype=np.uint64)]
    for x in xs:
        assert hc.mix64_inv(hc.mix64(x)) == x and hc.mix64(hc.mix64_inv(x)) == x
    assert (hc.MIX_A * hc.MIX_A_INV) & hc.M64 == 1 and (hc.MIX_B * hc.MIX_B_INV) & hc.M64 == 1
    assert (hc.FIB * hc.FIB_INV) & 0xFFFFFFFF == 1
    # splitmix64's first outputs from state 0 (Vigna's reference generator: state += 0x9E3779B97F4A7C15, then this finaliser)
    assert hc.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF and hc.mix64((2 * 0x9E3779B97F4A7C15) & hc.M64) == 0x6E789E6AA1B965F4
    arr = np.array(xs[:1000], dtype=np.uint64)
    assert [int(v) for v in hc.mix64_np(arr)] == [hc.mix64(x) for x in xs[:1000]]


def test_hash_bytes_is_fnv1a_then_the_length():
    assert hc.hash_bytes(b"") == hc.mix64(0xCBF29CE484222325)
    assert hc.hash_bytes(b"a") == hc.mix64(0xAF63DC4C8601EC8C ^ 1)           # FNV-1a 64 of "a" (the published test vector)
    assert hc.hash_bytes("foobar") == hc.mix64(0x85944171F73967E8 ^ 6)
    assert hc.hash_bytes("été") == hc.hash_bytes("été".encode())
    texts = [b"", b"a", b"foobar", b"s12345", b"x" * 70]
    h, lens = hc._fnv_np(np.full(len(texts), hc.FNV_BASIS, np.uint64), texts)
    assert [hc.mix64(int(a) ^ int(b)) for a, b in zip(h, lens)] == [hc.hash_bytes(t) for t in texts]


def test_pow2_at_least_has_a_floor_of_1024():
    assert [hc.pow2_at_least(v) for v in (0, 1, 1024, 1025, 12_000, 16_384, 16_385)] == [1024, 1024, 1024, 2048, 16_384, 16_384, 32_768]


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("low", LOWS)
def test_tag_cluster_one_tag_one_home(tag, low):
    keys = hc.tag_cluster(tag, low, 256)
    assert len(set(keys)) == 256 and all(-2**63 < k < 2**63 for k in keys)
    for k in keys:
        h = hc.mix64(k)
        assert h >> 32 == tag and h & 0xFFFFFF == low
        for cap in CAPS:
            assert hc.home(h, cap) == low & (cap - 1)
    if low == 0xFFFFFF:
        assert all(hc.home(hc.mix64(keys[0]), cap) == cap - 1 for cap in CAPS)       # the last slot of every table: the run wraps


@pytest.mark.parametrize("low", LOWS)
def test_home_cluster_one_home_different_tags(low):
    keys = hc.home_cluster(low, 5000)
    assert len(set(keys)) == 5000
    hs = [hc.mix64(k) for k in keys]
    assert all(h & 0xFFFFFF == low for h in hs) and len({h >> 32 for h in hs}) == 5000
    other = hc.home_cluster(low, 300, first=5000)
    assert not set(other) & set(keys)
    for d in (1, 3, 200):
        b = hc.behind(low, d, 40)
        assert not set(b) & set(keys) and all(hc.mix64(k) & 0xFFFFFF == (low + d) & 0xFFFFFF for k in b)
        assert all(hc.home(hc.mix64(k), 8192) == ((low & 8191) + d) & 8191 for k in b)


def test_key_tuple_hash_and_the_steered_last_column():
    # one Int64 column: seed, one step
    assert hc.key_tuple_hash([5]) == hc.mix64(((hc.TUPLE_SEED * hc.FNV_PRIME) & hc.M64) ^ 5)
    assert hc.key_tuple_hash([-1]) == hc.mix64(((hc.TUPLE_SEED * hc.FNV_PRIME) & hc.M64) ^ hc.M64)          # an Int32 -1 is widened with its sign
    assert hc.key_tuple_hash([None, 7]) == hc.tuple_step(hc.tuple_step(hc.TUPLE_SEED, hc.NULL_MARK), 7)
    assert hc.key_tuple_hash([7, None]) == hc.tuple_step(hc.tuple_step(hc.TUPLE_SEED, 7), (2 * hc.NULL_MARK) & hc.M64)
    assert hc.key_tuple_hash(["ab", 7]) == hc.tuple_step(hc.tuple_step(hc.TUPLE_SEED, hc.hash_bytes("ab")), 7)
    seen = set()
    for tag in TAGS:
        for low in LOWS:
            for m, first in enumerate([3, -2**62, None, "", "name-17", "x" * 70]):
                target = (tag << 32) | (m << 24) | low
                v = hc.steer_last_i64(hc.prefix_hash([first]), target)
                assert -2**63 < v < 2**63 and hc.key_tuple_hash([first, v]) == target
                seen.add((first, v))
    assert len(seen) == len(TAGS) * len(LOWS) * 6
    # three columns: the prefix is whatever stands before the last
    v = hc.steer_last_i64(hc.prefix_hash(["a", None]), 0xFFFFFFFF00FFFFFF)
    assert hc.key_tuple_hash(["a", None, v]) == 0xFFFFFFFF00FFFFFF


def test_same_hash_pairs_have_identical_64_bit_hashes():
    for x in (12345, -7, 2**62 + 3):
        pairs = hc.same_hash_pairs(x, range(200))
        assert pairs[0] == (0, x) and len({v for _, v in pairs}) == 200
        assert {hc.distinct_pair_hash(g, v) for g, v in pairs} == {hc.mix64(x)}
    assert hc.distinct_pair_hash(3, -1) == hc.mix64((hc.M64 + 3 * hc.PAIR_STEP) & hc.M64)


def test_fib_cluster_shares_its_home_in_every_table_of_up_to_2_20_slots():
    for top in (0, 0xFFFFF, 0x5A5A5):
        keys = hc.fib_cluster(top, 4096)
        assert len(set(keys)) == 4096 and all(0 <= k < 2**32 for k in keys)
        for cap in (1024, 1536, 4096, 100_003, 1 << 20):          # (slot_of takes any size, not only powers of two)
            assert len({hc.slot_of(k, cap) for k in keys}) == 1
        assert hc.slot_of(keys[0], 1 << 20) == top
    assert hc.slot_of(1, 1024) == (hc.FIB * 1024) >> 32


@pytest.mark.parametrize("cap", [8192, 16384, 65536])
def test_search_i32_finds_home_clusters_at_the_exact_size(cap):
    want = 16 if cap > 16384 else 64
    clusters = hc.search_i32(cap, want, count=4)
    flat = [v for c in clusters for v in c]
    assert len(clusters) == 4 and all(len(c) == want for c in clusters) and len(set(flat)) == len(flat)
    assert all(-2**31 <= v < 2**31 for v in flat)
    for c in clusters:
        assert len({hc.home(hc.mix64(v), cap) for v in c}) == 1
    assert len({hc.home(hc.mix64(c[0]), cap) for c in clusters}) == 4


@pytest.mark.parametrize("cap", [8192, 16384])
def test_search_utf8_finds_home_clusters_with_last_byte_twins_and_two_lengths(cap):
    clusters = hc.search_utf8(cap, 16, count=3)
    flat = [s for c in clusters for s in c]
    assert len(clusters) == 3 and len(set(flat)) == len(flat)
    for c in clusters:
        assert len(c) >= 16 and len({hc.home(hc.hash_bytes(s), cap) for s in c}) == 1
        assert len({len(s) for s in c}) >= 2
        assert any(a != b and a[:-1] == b[:-1] for a in c for b in c)


def test_search_utf8_run_fills_neighbouring_slots():
    cap = 16384
    texts = hc.search_utf8_run(cap, 1500, 2)
    assert len(set(texts)) == 3000
    homes = [hc.home(hc.hash_bytes(s), cap) for s in texts]
    assert homes[0] == cap - 750 and all(homes[2 * k] == homes[2 * k + 1] == (cap - 750 + k) % cap for k in range(1500))


@pytest.mark.parametrize("cap", [8192, 16384])
def test_search_pairs_finds_home_clusters_of_int32_utf8_pairs(cap):
    clusters = hc.search_pairs(cap, 16, count=3)
    flat = [p for c in clusters for p in c]
    assert len(clusters) == 3 and all(len(c) == 16 for c in clusters) and len(set(flat)) == len(flat)
    for c in clusters:
        assert len({hc.home(hc.distinct_i32_utf8_hash(k, s), cap) for k, s in c}) == 1
    assert hc.distinct_i32_utf8_hash(-1, "") == hc.mix64(hc.FNV_BASIS ^ 0xFFFFFFFF)
