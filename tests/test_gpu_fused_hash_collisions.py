"""Crafted hash collisions for the tables of hashtab.hpp behind the fused queries: q3's hash path (built in LDS, and in global memory behind a lost
bet), q8's hash path grouped by bucket, q13's side-input join (probed from its LDS copy and from global memory) -- window by window against the oracle.

hashtab.hpp's slot_of is (key * kFibHash * cap) >> 32: the ids ((T << 12 | j) * kFibHash^-1) mod 2^32 (tests/hash_craft.py fib_cluster, proven by
tests/test_hash_craft.py) share their home slot in EVERY table of up to 2^20 slots, whatever its size -- and q8's bucket and the slots inside it,
which are the top bits of key * kFibHash.  Random and generator ids give runs of two or three; here 64 ids meet in one slot, with duplicates on
both sides, at the table's last slot (T = 0xFFFFF: the run wraps) and its first, and probes that are absent but homed inside a cluster.  No cluster
is larger than 64: the paths' retries with larger tables are not the subject."""
import numpy as np
import pytest

import hash_craft as hc
import oracle
import test_gpu_parity as P

pytestmark = pytest.mark.gpu
TOPS = [0xFFFFF, 0, 0x5A5A5]          # the last slot of every table, the first, one in between


def _ids(top, lo, hi):
    ids = np.array(hc.fib_cluster(top, hi)[lo:hi], dtype=np.uint32).astype(np.int32)
    assert -1 not in ids
    return ids


def _text(rows):
    return oracle.Utf8(np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int32), np.frombuffer(b"".join(rows) or b"\0", np.uint8).copy())


def _profiled(c, call):
    c.profile_reset()
    c.profile(True)
    try:
        out = call()
        ran = set(c.profile_read())
    finally:
        c.profile(False)
    return out, ran


def test_q3_hash_path_with_persons_and_sellers_that_share_a_home():
    """q3_window_join_lds_kernel and, behind a lost bet, the global tables of q3_build_kernel / q3_probe_count_kernel: in every window 64 persons per
    cluster share ONE home slot (16 of them twice: duplicates on the build side), the auctions name them many times, and sellers that no person
    has but whose home lies inside the cluster.  Sparse ids in no order: only the hash path can answer."""
    from flock_amd import Auctions, GpuContext, Persons, WindowSchedule
    c = GpuContext(0)
    rng = np.random.default_rng(2301)
    npn, na = 40_000, 120_000
    p_id = P._sorted_keys(rng, npn, 50_000)
    held = np.zeros(npn, bool)
    for w in range(4):                                                 # the finest windows: 10 000 persons each
        at = w * 10_000 + rng.choice(10_000, 80 * len(TOPS), replace=False)
        for k, top in enumerate(TOPS):
            ids = _ids(top, 0, 64)
            p_id[at[80 * k:80 * (k + 1)]] = np.concatenate([ids, ids[:16]])
        held[at] = True
    nm = [b"n%d" % (i % 911) for i in range(npn)]
    name = _text(nm)
    seller = rng.choice(p_id, na).astype(np.int32)
    hot = np.concatenate([_ids(top, 0, 128) for top in TOPS])         # present ids and, from 64 on, absent ones of the same home
    spots = rng.choice(na, 24_000, replace=False)
    seller[spots] = rng.choice(hot, len(spots))
    category = rng.integers(10, 12, na).astype(np.int32)
    a_id = (np.arange(na) * 3 + 1).astype(np.int32)
    # (20 000 persons into the LDS-sized table: the bet is lost, global tables; the same size again: no bet; smaller windows: the LDS build)
    plan = (([b"or"], [0, 20_000, npn], {"q3_window_join_lds_kernel": True, "q3_probe_count_kernel": True}),
            ([b"or", b"wa", b"tx", b"id"], [0, 20_000, npn], {"q3_window_join_lds_kernel": False, "q3_probe_count_kernel": True}),
            ([b"or", b"wa"], [0, 9_000, 20_000, 31_000, npn], {"q3_window_join_lds_kernel": True, "q3_probe_count_kernel": False}))
    for states, edges, expect in plan:
        st = rng.choice(np.array(states, dtype=object), npn)
        st[held] = b"or"                                               # the clusters pass the state filter: they are IN the tables
        state = _text(list(st))
        n_w = len(edges) - 1
        pw = WindowSchedule(np.array(edges), np.arange(n_w), np.arange(1, n_w + 1))
        aw = WindowSchedule(np.linspace(0, na, n_w + 1).astype(np.int64), np.arange(n_w), np.arange(1, n_w + 1))
        out, ran = _profiled(c, lambda: c.q3_join(Auctions(P._dev(a_id), P._dev(seller), P._dev(category), na), aw,
                                                  Persons(P._dev(p_id), P._utf8(name), P._utf8(name), P._utf8(state), npn), pw).to_host())
        for k, want in expect.items():
            assert (k in ran) == want, (states, k, sorted(ran))
        off, total = out["offsets"], 0
        for w in range(n_w):
            (alo, ahi), (plo, phi) = aw.window_rows(w), pw.window_rows(w)
            ar, pr = oracle.q3_join(seller[alo:ahi], category[alo:ahi], p_id[plo:phi], state.slice(plo, phi))
            sl = slice(off[w], off[w + 1])
            assert sorted(zip((out["auction_row"][sl] - alo).tolist(), (out["person_row"][sl] - plo).tolist())) == sorted(zip(ar.tolist(), pr.tolist())), (states, w)
            total += len(ar)
        assert total == len(out["a_id"]) > 5000
    c.close()


def test_q8_hash_path_clusters_in_one_bucket_and_one_home():
    """q8_bucket_join_kernel: per cluster 64 DISTINCT sellers in ONE bucket and ONE home slot of its seller set (32 of them persons, 32 sellers nobody
    is), 48 person ids there of which 32 sell -- each under three names, so that the 64 further names meet in ONE home slot of the bucket's table
    of further names -- and exact duplicates of persons.  In both windows, with ids over the whole int32 range in no order around them."""
    from flock_amd import Auctions, GpuContext, Persons, WindowSchedule
    c = GpuContext(0)
    rng = np.random.default_rng(2302)
    npn, na = 60_000, 100_000
    pw = WindowSchedule(np.array([0, 30_000, npn]), np.arange(2), np.arange(1, 3))
    aw = WindowSchedule(np.array([0, 50_000, na]), np.arange(2), np.arange(1, 3))
    log2nb = P._q8_part_log2(30_000, 50_000)
    assert 4 <= log2nb <= 8                                           # bucket and both slot numbers are bits of the 20 the cluster shares
    p_id = rng.integers(-2**31, 2**31 - 1, npn).astype(np.int32)
    nm = [b"f%d" % i for i in range(npn)]
    seller = rng.choice(p_id, na).astype(np.int32)
    for w in range(2):
        rows = w * 30_000 + rng.choice(30_000, 200 * len(TOPS), replace=False)
        spots = w * 50_000 + rng.choice(50_000, 1_000 * len(TOPS), replace=False)
        for k, top in enumerate(TOPS):
            ids, mine = _ids(top, 0, 128), rows[200 * k:200 * (k + 1)]
            buckets = P._q8_part_bucket(ids, log2nb)
            assert len(set(buckets.tolist())) == 1 and len({hc.slot_of(int(i) & 0xFFFFFFFF, 1 << (log2nb + 12)) for i in ids}) == 1
            persons = np.concatenate([ids[:48], ids[:32], ids[:32], ids[:40]])              # 152 rows: three names under 32 ids, then duplicates
            p_id[mine[:152]] = persons
            for j in range(112, 152):                                                      # the last 40: the name of the id's first person
                nm[mine[j]] = nm[mine[j - 112]]
            seller[spots[1_000 * k:1_000 * (k + 1)]] = rng.choice(np.concatenate([ids[:32], ids[96:128]]), 1_000)
    name = _text(nm)
    per = Persons(P._dev(p_id), P._utf8(name), None, None, npn)
    auc = Auctions(None, P._dev(seller), None, na)
    for rep in range(2):
        out, ran = _profiled(c, lambda: c.q8_join(per, pw, auc, aw).to_host())
        assert "q8_bucket_join_kernel" in ran and "q8_persons_general_kernel" not in ran, sorted(ran)
        assert P._q8_check(out, pw, aw, p_id, name, nm, seller, rep) > 10_000
    c.close()


@pytest.mark.parametrize("n_side", [8191, 8192])
def test_q13_side_input_join_through_clusters(n_side):
    """q13's side table has 2 * rows + 1 slots: 8191 side rows are probed from the LDS copy (find_lds, 16383 slots), 8192 from global memory
    (find_global).  Side keys in clusters of 64 that share a home, 16 of each twice; bid keys present, and absent but homed inside a cluster.  The
    side keys span more than 2^31 ids: no bitmap, every bid goes through the table."""
    from flock_amd import Bids, GpuContext, WindowSchedule
    c = GpuContext(0)
    rng = np.random.default_rng(n_side)
    key = rng.integers(-2**31, 2**31 - 1, n_side).astype(np.int32)
    key[:2] = [-2**31 + 5, 2**31 - 7]
    at = 2 + rng.choice(n_side - 2, 80 * len(TOPS), replace=False)
    for k, top in enumerate(TOPS):
        ids = _ids(top, 0, 64)
        key[at[80 * k:80 * (k + 1)]] = np.concatenate([ids, ids[:16]])
    value = rng.integers(-2**31, 2**31 - 1, n_side).astype(np.int32)
    n_bids = 60_000
    hot = np.concatenate([_ids(top, 0, 128) for top in TOPS])
    auction = np.where(rng.random(n_bids) < 0.3, rng.choice(hot, n_bids), np.where(rng.random(n_bids) < 0.5, rng.choice(key, n_bids),
                                                                                    rng.integers(-2**31, 2**31 - 1, n_bids))).astype(np.int32)
    cols = {"auction": auction, "bidder": rng.integers(0, 1000, n_bids).astype(np.int32), "price": rng.integers(0, 10**6, n_bids).astype(np.int32),
            "b_date_time": np.arange(n_bids, dtype=np.int64) * 7}
    bids = Bids(P._dev(cols["auction"]), P._dev(cols["bidder"]), P._dev(cols["price"]), P._dev(cols["b_date_time"]), n_bids)
    sched = WindowSchedule(np.array([0, 20_000, 40_000, n_bids]), np.arange(3), np.arange(1, 4))
    out, ran = _profiled(c, lambda: c.q13_side_join(bids, sched, P._dev(key), P._dev(value)).to_host())
    assert "q13_build_kernel" in ran and "q13_probe_count_kernel" in ran and "q13_flag_kernel" not in ran, sorted(ran)
    off, total = out["offsets"], 0
    for w in range(3):
        lo, hi = sched.window_rows(w)
        br, sr = oracle.q13_side_join(auction[lo:hi], key)
        sl = slice(off[w], off[w + 1])
        assert sorted(zip((out["bid_row"][sl] - lo).tolist(), out["side_row"][sl].tolist())) == sorted(zip(br.tolist(), sr.tolist())), w
        assert (np.diff(out["bid_row"][sl].astype(np.int64)) >= 0).all()
        rows = out["bid_row"][sl]
        for k in ("auction", "bidder", "price", "b_date_time"):
            assert np.array_equal(out[k][sl], cols[k][rows]), (w, k)
        assert np.array_equal(out["value"][sl], value[out["side_row"][sl]])
        total += len(br)
    assert total == len(out["value"]) > 10_000
    c.close()
