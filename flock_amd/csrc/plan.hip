// Plan-level C ABI (include/flockgpu_plan.h): serde_json physical plan in, Arrow C Data Interface batches in / out.
//   feed_data_sources  flock/src/runtime/context.rs:257-325   -> flockgpu_plan_feed (plan_feed.hip, as all of ingest)
//   execute            flock/src/runtime/context.rs:172-191   -> flockgpu_plan_execute
//   execute_partitioned context.rs:197-216 (chosen by is_shuffling, context.rs:328-337; flock-function/src/aws/actor.rs:60-66)
//                                                             -> flockgpu_plan_execute_partitioned
//   clean_data_sources context.rs:227-254                     -> flockgpu_plan_reset (plan_feed.hip)
// The plan is parsed into the operator tree of plan_ir.hpp.  Sub-trees that are one of the NEXMark pipelines run as the
// fused kernels of flockgpu.h (q2 filter, q3 / q8 / q13 joins, q5 / q7 aggregates, the Partial COUNT of q5.dag);
// every other node -- the STAGE plans either side of a `RepartitionExec Hash` -- runs on the generic operators of
// relops.hpp.  Host-side code only; all compute goes through those two layers.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <map>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>

#include "../../include/flockgpu_plan.h"
#include "plan_state.hpp"
#include "comm_table.hpp"
#include "cross.hpp"
#include "union.hpp"
#include "pred.hpp"
#include "distinct.hpp"
#include "groupwide.hpp"
#include "reduce.hpp"
#include "strmatch.hpp"
#include "textsel.hpp"
#include "valprog.hpp"

using namespace flockgpu;
using namespace flockgpu::ir;
using namespace flockgpu::plan_detail;

namespace {
// ------------------------------------------------------------------ pinned host memory, pooled
// Output batches live in pinned host memory (one block per execute); blocks return to a process-wide pool when the
// consumer calls the Arrow release callback (possibly from another thread, possibly after the ctx is gone).
struct PinnedPool {
    std::mutex mu;
    std::vector<std::pair<size_t, void *>> free_blocks;
    size_t held = 0;
    static constexpr size_t kMaxHeld = size_t(2) << 30;
    void *get(size_t bytes, size_t *cap) {
        {
            std::lock_guard<std::mutex> g(mu);
            size_t best = free_blocks.size();
            for (size_t i = 0; i < free_blocks.size(); ++i)
                if (free_blocks[i].first >= bytes && free_blocks[i].first <= bytes * 2 + (1 << 20) &&
                    (best == free_blocks.size() || free_blocks[i].first < free_blocks[best].first))
                    best = i;
            if (best != free_blocks.size()) {
                auto b = free_blocks[best];
                free_blocks.erase(free_blocks.begin() + (long)best);
                held -= b.first;
                *cap = b.first;
                return b.second;
            }
        }
        size_t want = std::max<size_t>(bytes + bytes / 8, 4096);
        want = (want + 4095) & ~size_t(4095);
        void *p = nullptr;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return nullptr;
        *cap = want;
        return p;
    }
    void put(void *p, size_t cap) {
        {
            std::lock_guard<std::mutex> g(mu);
            if (held + cap <= kMaxHeld) {
                free_blocks.emplace_back(cap, p);
                held += cap;
                return;
            }
        }
        (void)hipHostFree(p);
    }
};
PinnedPool &pool() {
    static PinnedPool *p = new PinnedPool();  // never destroyed: release callbacks may run during process exit
    return *p;
}
struct HostBlock {  // shared by the partitions of one execute
    void *ptr = nullptr;
    size_t cap = 0;
    ~HostBlock() {
        if (ptr) pool().put(ptr, cap);
    }
};

// ------------------------------------------------------------------ fused-pipeline recognition (structure only)
struct Peeled {
    const Node *n = nullptr;
    std::vector<int> map;  // output column of the peeled-from node -> column of n (-1: computed)
};
// Follows projections that only select / rename columns and hash repartitions (no effect on the row multiset).
Peeled peel(const Node *n) {
    Peeled p;
    p.n = n;
    p.map.resize(n->schema.size());
    for (size_t i = 0; i < p.map.size(); ++i) p.map[i] = (int)i;
    for (;;) {
        if (p.n->kind == NKind::Repartition) {
            p.n = p.n->in[0].get();
            continue;
        }
        if (p.n->kind == NKind::Project) {
            bool pure = true;
            for (auto &e : p.n->proj) pure = pure && e.first->kind == EKind::Col;
            if (!pure) return p;
            for (auto &m : p.map)
                if (m >= 0) m = p.n->proj[(size_t)m].first->col;
            p.n = p.n->in[0].get();
            continue;
        }
        return p;
    }
}
const Expr *uncast(const Expr *e) {
    while (e && e->kind == EKind::Cast && !e->text_num && (e->cast_to == ColType::I64 || e->cast_to == ColType::F64)) e = e->l.get();   // (a parse of text is no such cast)
    return e;
}
bool is_bin(const Expr *e, const char *op) { return e && e->kind == EKind::Bin && e->s == op; }

// Logical aggregate: Final / FinalPartitioned over (peeled) Partial with the same shape, or a single stage.
// Returns the node below the lowest aggregate stage and the group / argument columns in ITS schema.
struct LogicalAgg {
    const Node *below = nullptr;
    std::vector<int> group;
    std::vector<AggFn> fns;
    std::vector<int> args;
};
bool logical_agg(const Node *n, LogicalAgg *out) {
    if (n->kind != NKind::Aggregate || n->single_pass) return false;   // (a single pass -- a node with a distinct count -- is no fused pipeline's)
    const Node *low = n;
    if (n->mode != AggMode::Partial) {
        Peeled p = peel(n->in[0].get());
        if (p.n->kind == NKind::Aggregate && p.n->mode == AggMode::Partial && p.n->group.size() == n->group.size() && p.n->aggs.size() == n->aggs.size()) {
            // the final stage must read the partial stage's columns in place
            for (size_t g = 0; g < n->group.size(); ++g)
                if (p.map[(size_t)n->group[g]] != (int)g) return false;
            int state_at = (int)n->group.size();
            for (size_t a = 0; a < n->aggs.size(); ++a) {
                if (p.map[(size_t)n->aggs[a].arg] != state_at || p.n->aggs[a].fn != n->aggs[a].fn) return false;
                if (n->aggs[a].arg2 >= 0 && p.map[(size_t)n->aggs[a].arg2] != state_at + 1) return false;
                state_at += agg_state_cols(n->aggs[a].fn);
            }
            low = p.n;
        } else {
            return false;  // a lone final stage (a stage plan): generic
        }
    }
    out->below = low->in[0].get();
    out->group = low->group;
    for (auto &a : low->aggs) {
        out->fns.push_back(a.fn);
        out->args.push_back(a.arg);
    }
    return true;
}
const Node *as_scan(const Node *n, std::vector<int> *map) {
    Peeled p = peel(n);
    if (p.n->kind != NKind::Scan) return nullptr;
    if (map) *map = p.map;
    return p.n;
}
bool req_subset(const Node *n, const std::vector<int> &allowed) {
    for (size_t i = 0; i < n->required.size(); ++i)
        if (n->required[i] && std::find(allowed.begin(), allowed.end(), (int)i) == allowed.end()) return false;
    return true;
}

// Q of q4.sql / q9.sql: MAX(price) per auction [, category] over auction JOIN bid ON a_id = auction WHERE b_date_time BETWEEN
// a_date_time AND expires (planner.rs:218-256 stages 0-2; BETWEEN arrives as `x >= lo AND x <= hi`).
struct WinningBids {
    const Node *auction_scan = nullptr, *bid_scan = nullptr;
    int a_id = -1, a_dt = -1, a_exp = -1, a_cat = -1;  // columns of the auction leaf
    int b_auction = -1, b_price = -1, b_dt = -1;       // columns of the bid leaf
};
bool match_winning_bids(const Node *agg, bool with_category, WinningBids *w) {
    LogicalAgg la;
    if (!logical_agg(agg, &la) || la.fns != std::vector<AggFn>{AggFn::Max} || la.group.size() != (with_category ? 2u : 1u)) return false;
    Peeled pf = peel(la.below);
    if (pf.n->kind != NKind::Filter) return false;
    Peeled pj = peel(pf.n->in[0].get());
    if (pj.n->kind != NKind::Join || pj.n->join_type != JoinType::Inner || pj.n->on.size() != 1) return false;
    const Node *J = pj.n;
    const int nl = (int)J->in[0]->schema.size();
    auto to_join = [&](int below_col) {  // column of la.below -> column of the join's output
        const int f = pf.map[(size_t)below_col];
        return f < 0 ? -1 : pj.map[(size_t)f];
    };
    // b_date_time >= a_date_time AND b_date_time <= expires (either order of the conjuncts)
    const Expr *p = pf.n->pred.get();
    if (!is_bin(p, "And")) return false;
    int x = -1, lo = -1, hi = -1;
    for (const Expr *c : {p->l.get(), p->r.get()}) {
        if (!c || c->kind != EKind::Bin) return false;
        const Expr *a = uncast(c->l.get()), *b = uncast(c->r.get());
        if (a->kind != EKind::Col || b->kind != EKind::Col) return false;
        int cx, bound;
        bool is_lo;
        if (c->s == "GtEq") { cx = a->col; bound = b->col; is_lo = true; }
        else if (c->s == "LtEq") { cx = a->col; bound = b->col; is_lo = false; }
        else return false;
        if (x >= 0 && x != cx) return false;
        x = cx;
        (is_lo ? lo : hi) = bound;
    }
    if (x < 0 || lo < 0 || hi < 0) return false;
    x = pj.map[(size_t)x]; lo = pj.map[(size_t)lo]; hi = pj.map[(size_t)hi];
    const int key = to_join(la.group[0]), cat = with_category ? to_join(la.group[1]) : -1, price = to_join(la.args[0]);
    if (x < nl || lo < 0 || lo >= nl || hi < 0 || hi >= nl || price < nl || key != J->on[0].l || (with_category && (cat < 0 || cat >= nl))) return false;
    std::vector<int> lmap, rmap;
    w->auction_scan = as_scan(J->in[0].get(), &lmap);
    w->bid_scan = as_scan(J->in[1].get(), &rmap);
    if (!w->auction_scan || !w->bid_scan) return false;
    w->a_id = lmap[(size_t)J->on[0].l];
    w->a_dt = lmap[(size_t)lo];
    w->a_exp = lmap[(size_t)hi];
    w->a_cat = with_category ? lmap[(size_t)cat] : -1;
    w->b_auction = rmap[(size_t)J->on[0].r];
    w->b_price = rmap[(size_t)(price - nl)];
    w->b_dt = rmap[(size_t)(x - nl)];
    auto is = [](const Node *scan, int c, ColType t, bool ts) { return c >= 0 && scan->schema[(size_t)c].type == t && scan->schema[(size_t)c].is_ts == ts; };
    return is(w->auction_scan, w->a_id, ColType::I32, false) && is(w->auction_scan, w->a_dt, ColType::I64, true) &&
           is(w->auction_scan, w->a_exp, ColType::I64, true) && (!with_category || is(w->auction_scan, w->a_cat, ColType::I32, false)) &&
           is(w->bid_scan, w->b_auction, ColType::I32, false) && is(w->bid_scan, w->b_price, ColType::I32, false) && is(w->bid_scan, w->b_dt, ColType::I64, true);
}

void recognise_fused(flockgpu_plan *pl, const Node *n) {
    for (auto &c : n->in) recognise_fused(pl, c.get());
    FusedInfo &fi = pl->fused[(size_t)n->id];
    if (pl->generic_only) return;
    auto leaf_schema = [&](const Node *scan) -> const std::vector<Field> & { return pl->ir.leaves[(size_t)scan->leaf].schema; };
    if (n->kind == NKind::Filter) {
        // ---- q2: [cast] col % m = 0 over a scan; the engine emits (that column, one more Int32 column)
        std::vector<int> map;
        const Node *scan = as_scan(n->in[0].get(), &map);
        const Expr *p = n->pred.get();
        if (scan && is_bin(p, "Eq") && uncast(p->r.get())->kind == EKind::LitI && uncast(p->r.get())->i == 0) {
            const Expr *m = uncast(p->l.get());
            if (is_bin(m, "Modulo") && uncast(m->l.get())->kind == EKind::Col && uncast(m->r.get())->kind == EKind::LitI) {
                const int kc = uncast(m->l.get())->col;
                const int64_t mod = uncast(m->r.get())->i;
                int other = -1, extra = 0;
                for (size_t i = 0; i < n->required.size(); ++i)
                    if (n->required[i] && (int)i != kc) { other = (int)i; ++extra; }
                const bool ok_types = n->schema[(size_t)kc].type == ColType::I32 && (other < 0 || n->schema[(size_t)other].type == ColType::I32);
                if (mod != 0 && extra <= 1 && ok_types && map[(size_t)kc] >= 0 && (other < 0 || map[(size_t)other] >= 0)) {
                    fi.kind = kQ2;
                    fi.leaf_a = scan->leaf;
                    fi.a_cols = {map[(size_t)kc], other < 0 ? map[(size_t)kc] : map[(size_t)other]};
                    fi.out_map.assign(n->schema.size(), -1);
                    fi.out_map[(size_t)kc] = 0;
                    if (other >= 0) fi.out_map[(size_t)other] = 1;
                    fi.lit = mod;
                }
            }
        }
        return;
    }
    if (n->kind == NKind::Aggregate) {
        // ---- Partial COUNT GROUP BY one Int32 column of a scan (stage 0 of q5.dag)
        std::vector<int> map;
        const Node *scan = as_scan(n->in[0].get(), &map);
        if (scan && n->mode == AggMode::Partial && n->group.size() == 1 && n->aggs.size() == 1 && n->aggs[0].fn == AggFn::Count &&
            n->in[0]->schema[(size_t)n->group[0]].type == ColType::I32 && map[(size_t)n->group[0]] >= 0) {
            fi.kind = kPartialCount;
            fi.leaf_a = scan->leaf;
            fi.a_cols = {map[(size_t)n->group[0]]};
            fi.out_map = {0, 1};
            return;
        }
        LogicalAgg top;
        if (n->mode == AggMode::Partial || !logical_agg(n, &top) || top.group.size() != 1 || top.fns.size() != 1) return;
        // ---- q4: AVG(final) GROUP BY category over Q (q4.sql; planner.rs:218-256)
        if (top.fns[0] == AggFn::Avg) {
            Peeled pq = peel(top.below);
            WinningBids w;
            if (match_winning_bids(pq.n, true, &w) && pq.map[(size_t)top.group[0]] == 1 && pq.map[(size_t)top.args[0]] == 2) {
                fi.kind = kQ4;
                fi.leaf_a = w.auction_scan->leaf;
                fi.leaf_b = w.bid_scan->leaf;
                fi.a_cols = {w.a_id, w.a_cat, w.a_dt, w.a_exp};
                fi.b_cols = {w.b_auction, w.b_price, w.b_dt};
                fi.out_map = {0, 1};
            }
            return;
        }
        // ---- YSB: COUNT(*) GROUP BY campaign_id over Filter(event_type = lit)(ad_event) JOIN campaign ON ad_id = c_ad_id
        // (ysb.sql; planner.rs:298-346)
        if (top.fns[0] == AggFn::Count && top.below->schema[(size_t)top.group[0]].type == ColType::UTF8) {
            Peeled pj = peel(top.below);
            if (pj.n->kind != NKind::Join || pj.n->join_type != JoinType::Inner || pj.n->on.size() != 1) return;
            const Node *J = pj.n;
            const int nl = (int)J->in[0]->schema.size();
            Peeled pl_ = peel(J->in[0].get());
            std::vector<int> lmap, rmap;
            const Node *rs = as_scan(J->in[1].get(), &rmap);
            if (pl_.n->kind != NKind::Filter || !rs) return;
            const Node *ls = as_scan(pl_.n->in[0].get(), &lmap);
            const Expr *p = pl_.n->pred.get();
            if (!ls || !is_bin(p, "Eq") || p->l->kind != EKind::Col || p->r->kind != EKind::LitS || p->r->s.size() > 40) return;
            const int grp = pj.map[(size_t)top.group[0]];
            const int ev_key = pl_.map[(size_t)J->on[0].l];
            if (grp < nl || ev_key < 0) return;
            const int ad = lmap[(size_t)ev_key], ty = lmap[(size_t)p->l->col], cad = rmap[(size_t)J->on[0].r], camp = rmap[(size_t)(grp - nl)];
            auto text = [](const Node *scan, int c) { return c >= 0 && scan->schema[(size_t)c].type == ColType::UTF8; };
            if (!text(ls, ad) || !text(ls, ty) || !text(rs, cad) || !text(rs, camp)) return;
            fi.kind = kYsb;
            fi.leaf_a = ls->leaf;
            fi.leaf_b = rs->leaf;
            fi.a_cols = {ad, ty};
            fi.b_cols = {cad, camp};
            fi.strs = {p->r->s};
            fi.out_map = {0, 1};
        }
        return;
    }
    if (n->kind != NKind::Join || n->join_type != JoinType::Inner) return;   // (a Semi / Anti look-alike of q3 / q8 / q9 runs on the generic operators)
    const Node *L = n->in[0].get(), *R = n->in[1].get();
    const size_t nl = L->schema.size();
    const KeyPair on = n->on[0];
    const Field &lk = L->schema[(size_t)on.l], &rk = R->schema[(size_t)on.r];
    if (n->on.size() > 2) return;   // (more than two key pairs: no fused pipeline reads a third one)
    if (n->on.size() == 2) {
        // ---- q9: bid JOIN Q ON auction = id AND price = final (q9.sql, q9_plan.fmt)
        std::vector<int> lmap;
        const Node *ls = as_scan(L, &lmap);
        Peeled pr = peel(R);
        WinningBids w;
        if (!ls || !match_winning_bids(pr.n, false, &w)) return;
        const auto &bs = pl->ir.leaves[(size_t)ls->leaf].schema;
        static const char *names[4] = {"auction", "bidder", "price", "b_date_time"};
        bool ok = bs.size() == 4 && lmap.size() == 4 && n->required.size() == 6;
        for (int i = 0; ok && i < 4; ++i)
            ok = bs[(size_t)i].name == names[i] && lmap[(size_t)i] == i && n->required[(size_t)i] && bs[(size_t)i].type == (i == 3 ? ColType::I64 : ColType::I32);
        // the pairs in either order: (auction, id = the group key) and (price, final = the maximum)
        int k_auction = on.l, k_id = pr.map[(size_t)on.r], k_price = n->on[1].l, k_final = pr.map[(size_t)n->on[1].r];
        if (k_auction == 2) { std::swap(k_auction, k_price); std::swap(k_id, k_final); }
        ok = ok && k_auction == 0 && k_price == 2 && k_id == 0 && k_final == 1;
        // the inner bid scan must be the same relation (the SQL scans `bid` twice)
        const auto &inner = pl->ir.leaves[(size_t)w.bid_scan->leaf].schema;
        ok = ok && inner[(size_t)w.b_auction].name == "auction" && inner[(size_t)w.b_price].name == "price" && inner[(size_t)w.b_dt].name == "b_date_time";
        if (ok) {
            fi.kind = kQ9;
            fi.leaf_a = w.auction_scan->leaf;
            fi.leaf_b = ls->leaf;
            fi.a_cols = {w.a_id, -1, w.a_dt, w.a_exp};
            fi.out_map = {0, 1, 2, 3, 0, 2};  // id equals auction, final equals price on every output row
        }
        return;
    }
    // ---- q3: Filter(int col = lit)(scan) JOIN Filter(utf8 col = a OR ...)(scan) on Int32 keys
    {
        Peeled pl_ = peel(L), pr = peel(R);
        if (pl_.n->kind == NKind::Filter && pr.n->kind == NKind::Filter && lk.type == ColType::I32 && rk.type == ColType::I32) {
            std::vector<int> lmap, rmap;
            const Node *ls = as_scan(pl_.n->in[0].get(), &lmap), *rs = as_scan(pr.n->in[0].get(), &rmap);
            const Expr *lp = pl_.n->pred.get();
            bool ok = ls && rs && is_bin(lp, "Eq") && uncast(lp->l.get())->kind == EKind::Col && uncast(lp->r.get())->kind == EKind::LitI;
            int cat_col = -1, state_col = -1;
            std::vector<std::string> states;
            if (ok) {
                cat_col = uncast(lp->l.get())->col;
                ok = pl_.n->schema[(size_t)cat_col].type == ColType::I32;
                std::vector<const Expr *> stack{pr.n->pred.get()};
                while (!stack.empty() && ok) {
                    const Expr *e = stack.back();
                    stack.pop_back();
                    if (is_bin(e, "Or")) { stack.push_back(e->r.get()); stack.push_back(e->l.get()); }
                    else if (is_bin(e, "Eq") && e->l->kind == EKind::Col && e->r->kind == EKind::LitS && (state_col < 0 || state_col == e->l->col) &&
                             pr.n->schema[(size_t)e->l->col].type == ColType::UTF8) { state_col = e->l->col; states.push_back(e->r->s); }
                    else ok = false;
                }
                ok = ok && !states.empty() && states.size() <= 8;
            }
            if (ok) {
                // required outputs: at most one Int32 column of the left side (-> the a_id slot), Utf8 columns of the right
                // side: the filter column (-> state slot) and up to two more (-> name, city slots)
                int a_id = -1;
                std::vector<int> texts;
                for (size_t i = 0; i < n->required.size() && ok; ++i) {
                    if (!n->required[i]) continue;
                    if (i < nl) {
                        const int c = pl_.map[i];
                        if (c < 0 || pl_.n->schema[(size_t)c].type != ColType::I32 || (a_id >= 0 && a_id != c)) ok = false;
                        else a_id = c;
                    } else {
                        const int c = pr.map[i - nl];
                        if (c < 0 || pr.n->schema[(size_t)c].type != ColType::UTF8) ok = false;
                        else if (c != state_col && std::find(texts.begin(), texts.end(), c) == texts.end()) texts.push_back(c);
                    }
                }
                ok = ok && texts.size() <= 2;
                const int lkey = pl_.map[(size_t)on.l], rkey = pr.map[(size_t)on.r];
                ok = ok && lkey >= 0 && rkey >= 0;
                if (ok) {
                    if (a_id < 0) a_id = lkey;
                    while (texts.size() < 2) texts.push_back(state_col);
                    auto to_leaf = [](const std::vector<int> &m, int c) { return m[(size_t)c]; };
                    fi.kind = kQ3;
                    fi.leaf_a = ls->leaf;
                    fi.leaf_b = rs->leaf;
                    fi.a_cols = {to_leaf(lmap, a_id), to_leaf(lmap, lkey), to_leaf(lmap, cat_col)};            // a_id, seller, category
                    fi.b_cols = {to_leaf(rmap, rkey), to_leaf(rmap, texts[0]), to_leaf(rmap, texts[1]), to_leaf(rmap, state_col)};  // p_id, name, city, state
                    ok = std::all_of(fi.a_cols.begin(), fi.a_cols.end(), [](int c) { return c >= 0; }) &&
                         std::all_of(fi.b_cols.begin(), fi.b_cols.end(), [](int c) { return c >= 0; });
                    fi.out_map.assign(n->schema.size(), -1);
                    for (size_t i = 0; i < n->required.size(); ++i) {
                        if (!n->required[i]) continue;
                        if (i < nl) fi.out_map[i] = 3;  // a_id slot
                        else {
                            const int c = pr.map[i - nl];
                            fi.out_map[i] = c == state_col ? 2 : (c == texts[0] ? 0 : 1);
                        }
                    }
                    fi.lit = uncast(lp->r.get())->i;
                    fi.strs = states;
                    if (!ok) fi = FusedInfo{};
                    else return;
                }
            }
        }
    }
    // ---- q8: DISTINCT (Int32, Utf8)(scan) JOIN DISTINCT (Int32)(scan)
    {
        Peeled pl_ = peel(L), pr = peel(R);
        LogicalAgg la, ra;
        if (logical_agg(pl_.n, &la) && logical_agg(pr.n, &ra) && la.fns.empty() && ra.fns.empty() && la.group.size() == 2 && ra.group.size() == 1) {
            std::vector<int> lmap, rmap;
            const Node *ls = as_scan(la.below, &lmap), *rs = as_scan(ra.below, &rmap);
            const int lkey = pl_.map[(size_t)on.l], rkey = pr.map[(size_t)on.r];
            if (ls && rs && lkey == 0 && rkey == 0 && la.below->schema[(size_t)la.group[0]].type == ColType::I32 &&
                la.below->schema[(size_t)la.group[1]].type == ColType::UTF8 && ra.below->schema[(size_t)ra.group[0]].type == ColType::I32 &&
                lmap[(size_t)la.group[0]] >= 0 && lmap[(size_t)la.group[1]] >= 0 && rmap[(size_t)ra.group[0]] >= 0) {
                bool ok = true;
                fi.out_map.assign(n->schema.size(), -1);
                for (size_t i = 0; i < n->required.size() && ok; ++i) {
                    if (!n->required[i]) continue;
                    const int c = i < nl ? pl_.map[i] : pr.map[i - nl];
                    if (c < 0) ok = false;
                    else fi.out_map[i] = i < nl ? c : 0;  // the seller column equals p_id on every output row
                }
                if (ok) {
                    fi.kind = kQ8;
                    fi.leaf_a = ls->leaf;
                    fi.leaf_b = rs->leaf;
                    fi.a_cols = {lmap[(size_t)la.group[0]], lmap[(size_t)la.group[1]]};
                    fi.b_cols = {rmap[(size_t)ra.group[0]]};
                    return;
                }
                fi = FusedInfo{};
            }
        }
    }
    // ---- q5: (COUNT GROUP BY k)(scan) JOIN (MAX over the same counts) ON count = max
    {
        Peeled pl_ = peel(L), pr = peel(R);
        LogicalAgg cnt, mx, cnt2;
        if (logical_agg(pl_.n, &cnt) && cnt.group.size() == 1 && cnt.fns == std::vector<AggFn>{AggFn::Count} && logical_agg(pr.n, &mx) &&
            mx.group.empty() && mx.fns == std::vector<AggFn>{AggFn::Max}) {
            Peeled below = peel(mx.below);
            std::vector<int> lmap, rmap;
            const Node *ls = as_scan(cnt.below, &lmap);
            if (ls && logical_agg(below.n, &cnt2) && cnt2.group.size() == 1 && cnt2.fns == std::vector<AggFn>{AggFn::Count} &&
                below.map[(size_t)mx.args[0]] == 1 /* MAX over the count column */) {
                const Node *rs = as_scan(cnt2.below, &rmap);
                const int lkey = pl_.map[(size_t)on.l];
                if (rs && lkey == 1 && pr.map[(size_t)on.r] == 0 && cnt.below->schema[(size_t)cnt.group[0]].type == ColType::I32 &&
                    lmap[(size_t)cnt.group[0]] >= 0 && rmap[(size_t)cnt2.group[0]] >= 0 &&
                    leaf_schema(ls)[(size_t)lmap[(size_t)cnt.group[0]]].name == leaf_schema(rs)[(size_t)rmap[(size_t)cnt2.group[0]]].name) {
                    bool ok = true;
                    fi.out_map.assign(n->schema.size(), -1);
                    for (size_t i = 0; i < n->required.size() && ok; ++i) {
                        if (!n->required[i]) continue;
                        const int c = i < nl ? pl_.map[i] : pr.map[i - nl];
                        if (c < 0) ok = false;
                        else fi.out_map[i] = i < nl ? c : 1;  // maxn equals num on every output row
                    }
                    if (ok) {
                        fi.kind = kQ5;
                        fi.leaf_a = ls->leaf;
                        fi.leaf_b = rs->leaf;  // the SQL scans the relation twice; whichever leaf was fed holds it
                        fi.a_cols = {lmap[(size_t)cnt.group[0]]};
                        fi.b_cols = {rmap[(size_t)cnt2.group[0]]};
                        return;
                    }
                    fi = FusedInfo{};
                }
            }
        }
    }
    // ---- q7: bid JOIN (MAX(price) over bid) ON price = maxprice; q13: bid JOIN side_input ON auction = key
    {
        std::vector<int> lmap, rmap;
        const Node *ls = as_scan(L, &lmap);
        auto names_are = [&](const Node *scan, std::initializer_list<const char *> want) {
            const auto &s = leaf_schema(scan);
            if (s.size() != want.size()) return false;
            size_t i = 0;
            for (const char *w : want)
                if (s[i++].name != w) return false;
            return true;
        };
        const bool bid4 = ls && names_are(ls, {"auction", "bidder", "price", "b_date_time"}) && leaf_schema(ls)[0].type == ColType::I32 &&
                          leaf_schema(ls)[1].type == ColType::I32 && leaf_schema(ls)[2].type == ColType::I32 && leaf_schema(ls)[3].type == ColType::I64;
        bool lmap_id = bid4;
        for (size_t i = 0; lmap_id && i < lmap.size(); ++i) lmap_id = lmap[i] == (int)i;
        if (lmap_id && lmap.size() == 4) {
            Peeled pr = peel(R);
            LogicalAgg mx;
            const bool all_bid = n->required[0] && n->required[1] && n->required[2] && n->required[3];  // the entry points read all four
            if (all_bid && on.l == 2 && logical_agg(pr.n, &mx) && mx.group.empty() && mx.fns == std::vector<AggFn>{AggFn::Max} && pr.map[(size_t)on.r] == 0) {
                const Node *rs = as_scan(mx.below, &rmap);
                if (rs && rmap[(size_t)mx.args[0]] >= 0 && leaf_schema(rs)[(size_t)rmap[(size_t)mx.args[0]]].name == "price" &&
                    leaf_schema(rs)[(size_t)rmap[(size_t)mx.args[0]]].type == ColType::I32) {
                    fi.kind = kQ7;
                    fi.leaf_a = ls->leaf;
                    fi.leaf_b = rs->leaf;
                    fi.out_map = {0, 1, 2, 3, 2};  // maxprice equals price on every output row
                    return;
                }
            }
            const Node *rs = as_scan(R, &rmap);
            if (all_bid && n->required.size() == 6 && n->required[5] && on.l == 0 && rs && names_are(rs, {"key", "value"}) && on.r == 0 && rmap == std::vector<int>{0, 1} &&
                leaf_schema(rs)[0].type == ColType::I32 && leaf_schema(rs)[1].type == ColType::I32) {
                fi.kind = kQ13;
                fi.leaf_a = ls->leaf;
                fi.leaf_b = rs->leaf;
                fi.out_map = {0, 1, 2, 3, 0, 4};  // key equals auction
                return;
            }
        }
    }
}

const char *fused_name(Fused f) {
    switch (f) {
        case kQ2: return "fused q2 filter (q1q2.hip)";
        case kQ3: return "fused q3 filter + hash join (q3.hip)";
        case kQ5: return "fused q5 count / max / select (q5.hip)";
        case kQ7: return "fused q7 max + select (q7.hip)";
        case kQ8: return "fused q8 distinct + join (q8.hip)";
        case kQ13: return "fused q13 side-input join (q13.hip)";
        case kPartialCount: return "fused Partial COUNT (q5.hip)";
        case kQ9: return "fused q9 winning bids (q4q9.hip; generic when the auction ids of a batch are not dense)";
        case kQ4: return "fused q4 average winning bid by category (q4q9.hip; generic when the auction ids of a batch are not dense)";
        case kYsb: return "fused YSB filter + join + count (ysb.hip)";
        default: return "generic (relops.hip)";
    }
}
// A filter's predicate as text -- printed for the predicates that hold a LIKE (the others' lines are what they were)
bool holds_like(const Expr *e) {
    if (!e) return false;
    if (e->kind == EKind::Bin && (e->s == "Like" || e->s == "NotLike")) return true;
    if (holds_like(e->l.get()) || holds_like(e->r.get())) return true;
    for (auto &x : e->list)
        if (holds_like(x.get())) return true;
    return false;
}
// ... or a scalar function: `Filter(floor(f) > 3)`, `Project(p_time = now())`
bool holds_func(const Expr *e) {
    if (!e) return false;
    if (e->kind == EKind::Func) return true;
    if (holds_func(e->l.get()) || holds_func(e->r.get())) return true;
    for (auto &x : e->list)
        if (holds_func(x.get())) return true;
    return false;
}
// ... or a cast of text to a number (textnum.hpp): `Filter(CAST(extra AS Int64) > 100)`
bool holds_text_num(const Expr *e) {
    if (!e) return false;
    if (e->kind == EKind::Cast && e->text_num) return true;
    if (holds_text_num(e->l.get()) || holds_text_num(e->r.get())) return true;
    for (auto &x : e->list)
        if (holds_text_num(x.get())) return true;
    return false;
}
void pred_text(const Expr *e, const std::vector<Field> &schema, std::ostringstream &os) {
    if (!e) { os << "?"; return; }
    static const std::pair<const char *, const char *> ops[] = {{"Eq", "="}, {"NotEq", "<>"}, {"Lt", "<"}, {"LtEq", "<="}, {"Gt", ">"}, {"GtEq", ">="}, {"And", "AND"}, {"Or", "OR"},
                                                                {"Like", "LIKE"}, {"NotLike", "NOT LIKE"}, {"Modulo", "%"}, {"Plus", "+"}, {"Minus", "-"}, {"Multiply", "*"}, {"Divide", "/"}};
    switch (e->kind) {
        case EKind::Col: os << schema[(size_t)e->col].name; return;
        case EKind::LitI: if (e->big_unsigned) os << (uint64_t)e->i; else os << e->i; return;
        case EKind::LitF: os << e->f; return;
        case EKind::LitS: os << "'" << e->s << "'"; return;
        case EKind::LitB: os << (e->i ? "TRUE" : "FALSE"); return;
        case EKind::LitNull: os << "NULL"; return;
        case EKind::Cast:
            if (e->text_num) {   // text made a number (textnum.hpp): CAST(left(credit_card, 4) AS Int32)
                static const char *types[] = {"Int32", "Int64", "UInt64", "Float64"};
                os << (e->try_cast ? "TRY_CAST(" : "CAST(");
                pred_text(e->l.get(), schema, os);
                os << " AS " << (e->cast_ts ? "Timestamp(ms)" : types[(int)e->cast_to & 3]) << ")";
                return;
            }
            if (e->num_text) {   // a number made text (numtext.hpp): CAST(price AS Utf8)
                os << (e->try_cast ? "TRY_CAST(" : "CAST(");
                pred_text(e->l.get(), schema, os);
                os << " AS Utf8)";
                return;
            }
            pred_text(e->l.get(), schema, os);   // (the value, not its conversion)
            return;
        case EKind::Neg: os << "-"; pred_text(e->l.get(), schema, os); return;
        case EKind::Not: os << "NOT ("; pred_text(e->l.get(), schema, os); os << ")"; return;
        case EKind::IsNull: pred_text(e->l.get(), schema, os); os << " IS NULL"; return;
        case EKind::IsNotNull: pred_text(e->l.get(), schema, os); os << " IS NOT NULL"; return;
        case EKind::InList:
            pred_text(e->l.get(), schema, os);
            os << (e->negated ? " NOT IN (" : " IN (");
            for (size_t i = 0; i < e->list.size(); ++i) { os << (i ? ", " : ""); pred_text(e->list[i].get(), schema, os); }
            os << ")";
            return;
        case EKind::Case: os << "CASE ..."; return;
        case EKind::Func: {
            if (fn_is_slice(e->fn)) {   // split_part(url, '/', 4)
                std::vector<std::string> names;
                for (auto &f : schema) names.push_back(f.name);
                os << slice_text(e, names);
                return;
            }
            static const char *units[] = {"second", "minute", "hour", "day", "week", "month", "year", "dow", "doy"};
            os << e->s << "(";
            if (e->i >= 0 && e->i < 9) os << "'" << units[e->i] << "', ";
            for (size_t i = 0; i < e->list.size(); ++i) { os << (i ? ", " : ""); pred_text(e->list[i].get(), schema, os); }
            os << ")";
            return;
        }
        case EKind::Bin: {
            const char *sym = e->s.c_str();
            for (auto &o : ops)
                if (e->s == o.first) sym = o.second;
            const bool junction = e->s == "And" || e->s == "Or";
            auto side = [&](const Expr *x) {
                const bool paren = junction && x && x->kind == EKind::Bin && (x->s == "And" || x->s == "Or") && x->s != e->s;
                if (paren) os << "(";
                pred_text(x, schema, os);
                if (paren) os << ")";
            };
            side(e->l.get());
            os << " " << sym << " ";
            side(e->r.get());
            return;
        }
    }
}
// keys_only: `n` lies under the right input of a Semi / Anti join, which reads that side for its key columns alone -- a scan there says which of its
// columns the plan uploads
void describe(const flockgpu_plan *pl, const Node *n, int depth, std::ostringstream &os, bool keys_only = false) {
    static const char *kinds[] = {"Scan", "Filter", "Project", "Aggregate", "Join", "Repartition", "Sort", "Limit", "Window", "Union"};
    const char *kind = kinds[(int)n->kind];
    if (n->kind == NKind::Join && n->join_type == JoinType::Semi) kind = "SemiJoin";
    if (n->kind == NKind::Join && n->join_type == JoinType::Anti) kind = "AntiJoin";
    if (n->kind == NKind::Join && n->join_type == JoinType::Cross) kind = "CrossJoin";
    os << std::string((size_t)depth * 2, ' ') << kind;
    if (n->kind == NKind::Aggregate) os << "(" << agg_mode_name(n->mode) << (n->single_pass ? ", single pass" : "") << ")";
    if (n->kind == NKind::Repartition) os << (n->hash_diff ? "(HashDiff, " : "(Hash, ") << n->n_parts << ")";
    if (n->kind == NKind::Scan) os << "(" << pl->ir.leaves[(size_t)n->leaf].relation << ")";
    if (n->kind == NKind::Limit) os << "(" << n->limit << ")";
    if (n->kind == NKind::Union) os << "(" << n->in.size() << " inputs)";
    if (n->kind == NKind::Filter && (holds_like(n->pred.get()) || holds_func(n->pred.get()) || holds_text_num(n->pred.get()))) {
        os << "(";
        pred_text(n->pred.get(), n->schema, os);
        os << ")";
    }
    if (n->kind == NKind::Project) {   // the columns computed with a scalar function, and the text-valued ones, as `name = expression`
        bool any = false;
        for (size_t i = 0; i < n->proj.size(); ++i) {
            const bool text = n->proj[i].first->kind != EKind::Col && i < n->schema.size() && n->schema[i].type == ColType::UTF8;   // 'bid', CASE ... (textsel.hpp)
            if (!holds_func(n->proj[i].first.get()) && !text && !holds_text_num(n->proj[i].first.get())) continue;
            os << (any ? ", " : "(") << n->proj[i].second << " = ";
            pred_text(n->proj[i].first.get(), n->in[0]->schema, os);
            any = true;
        }
        if (any) os << ")";
    }
    if (n->kind == NKind::Window)
        for (size_t w = 0; w < n->win.size(); ++w) {
            const WinExpr &x = n->win[w];
            const auto &ins = n->in[0]->schema;
            std::string fn = agg_fn_name(x.fn);
            for (auto &ch : fn) ch = (char)std::toupper((unsigned char)ch);
            os << (w ? ", " : "(");
            if (x.row_number) os << "ROW_NUMBER";
            else os << fn << "(" << (x.arg >= 0 ? ins[(size_t)x.arg].name : std::string("*")) << ")";
            os << " PARTITION BY";
            for (int c : x.part) os << " " << ins[(size_t)c].name;
            if (!x.order.empty()) {
                os << " ORDER BY";
                for (auto &o : x.order) os << " " << ins[(size_t)o.col].name << (o.descending ? " DESC" : "");
            }
            if (w + 1 == n->win.size()) os << ")";
        }
    if (n->kind == NKind::Sort) {
        os << "(";
        for (size_t i = 0; i < n->sort_cols.size(); ++i)
            os << (i ? ", " : "") << n->schema[(size_t)n->sort_cols[i].col].name << (n->sort_cols[i].descending ? " DESC" : " ASC");
        os << ")";
    }
    os << " [";
    for (size_t i = 0; i < n->schema.size(); ++i) os << (i ? ", " : "") << n->schema[i].name << ":" << type_name(n->schema[i]);
    os << "]";
    if (keys_only && n->kind == NKind::Scan) {
        const Leaf &lf = pl->ir.leaves[(size_t)n->leaf];
        os << "  reads [";
        bool first = true;
        for (size_t i = 0; i < lf.needed.size(); ++i)
            if (lf.needed[i]) { os << (first ? "" : ", ") << lf.schema[i].name; first = false; }
        os << "]";
    }
    const Fused f = pl->fused[(size_t)n->id].kind;
    if (n->kind != NKind::Scan && n->kind != NKind::Project && n->kind != NKind::Repartition) os << "  <- " << fused_name(f);
    os << "\n";
    if (f != kNone) return;  // the fused pipeline swallows the sub-tree
    for (size_t i = 0; i < n->in.size(); ++i)
        describe(pl, n->in[i].get(), depth + 1, os,   // (a cross join prunes both sides to what is read above it: its scans say what they upload, too)
                 // (so does a union: with it, leaves of one relation upload the columns ANY of them reads -- union.hpp A-U7)
                 keys_only || n->kind == NKind::Union || (n->kind == NKind::Join && (n->join_type == JoinType::Cross || (i == 1 && n->join_type != JoinType::Inner))));
}

// The whole plan is one NEXMark pipeline when, below pure projections, its root is a fused node (or q1's projection).
int classify(const flockgpu_plan *pl) {
    const Node *r = pl->ir.root.get();
    if (r->kind == NKind::Project) {
        int computed = 0;
        for (auto &e : r->proj) computed += e.first->kind != EKind::Col;
        if (computed == 1 && peel(r->in[0].get()).n->kind == NKind::Scan) return 1;
    }
    const Node *n = peel(r).n;
    switch (pl->fused[(size_t)n->id].kind) {
        case kQ2: return 2;
        case kQ3: return 3;
        case kQ5: return 5;
        case kQ7: return 7;
        case kQ8: return 8;
        case kQ13: return 13;
        case kQ9: return 9;
        case kQ4: return 4;
        case kYsb: return 100;  // not a NEXMark number: the Yahoo Streaming Benchmark's one query
        default: return 0;
    }
}

// ---- structural signatures (flockgpu_plan::twin_sig): everything about a sub-tree that decides the table it produces, leaves by their
// scanned columns (which leaf DATA a scan reads is decided per execute: Exec::resolve_leaf)
void expr_sig(const Expr *e, std::string *o) {
    if (!e) { *o += "~"; return; }
    uint64_t fbits = 0;   // (the literal's bits: std::to_string keeps six decimals, and two literals that differ beyond them are two tables)
    std::memcpy(&fbits, &e->f, sizeof fbits);
    *o += "(" + std::to_string((int)e->kind) + "," + std::to_string(e->col) + "," + std::to_string(e->i) + "," + std::to_string(fbits) + "," + e->s + "," +
          std::to_string((int)e->cast_to) + (e->negated ? "n" : "") + (e->big_unsigned ? "u" : "") + (e->try_cast ? "t" : "") + (e->cast_ts ? "s" : "") + "," + e->lit_kind;
    expr_sig(e->l.get(), o);
    expr_sig(e->r.get(), o);
    for (auto &x : e->list) expr_sig(x.get(), o);
    *o += ")";
}
void node_sig(const flockgpu_plan *pl, const Node *n, bool top, std::string *o, std::vector<int> *leaves) {
    *o += "[" + std::to_string((int)n->kind) + ":";
    for (size_t i = 0; i < n->schema.size(); ++i)
        *o += n->schema[i].name + "/" + std::to_string((int)n->schema[i].type) + (n->schema[i].is_ts ? "t" : "") + (n->schema[i].nullable ? "?" : "") +
              (!top && i < n->required.size() && n->required[i] ? "!" : "") + ",";   // (an Aggregate computes every output column: its own `required` does not matter)
    *o += "|" + std::to_string((int)n->mode) + (n->single_pass ? "s" : "") + "|";
    for (int c : n->group) *o += std::to_string(c) + ",";
    for (auto &a : n->aggs) *o += std::to_string((int)a.fn) + "." + std::to_string(a.arg) + "." + std::to_string(a.arg2) + "." + std::to_string((int)a.type) + ",";
    *o += "|";
    for (auto &k : n->on) *o += std::to_string(k.l) + "=" + std::to_string(k.r) + ",";   // (every key pair)
    *o += std::string(n->join_partitioned ? "p" : "") + (n->join_type == JoinType::Semi ? "s" : n->join_type == JoinType::Anti ? "a" : n->join_type == JoinType::Cross ? "x" : "") + "|";
    for (int c : n->hash_cols) *o += std::to_string(c) + ",";
    *o += std::to_string(n->n_parts) + (n->hash_diff ? "d" : "") + "|";
    for (auto &k : n->sort_cols) *o += std::to_string(k.col) + (k.descending ? "d" : "a") + (k.nulls_first ? "f" : "l") + ",";
    *o += std::to_string(n->limit) + "|";
    if (n->kind == NKind::Union) *o += "U" + std::to_string(n->in.size()) + "|";   // (its inputs follow below, in order)
    for (auto &x : n->win) {   // (Window: each column's function, argument, PARTITION BY and ORDER BY)
        *o += (x.row_number ? std::string("rn") : std::to_string((int)x.fn) + "." + std::to_string(x.arg) + "." + std::to_string((int)x.type)) + ":";
        for (int c : x.part) *o += std::to_string(c) + ",";
        *o += "/";
        for (auto &k : x.order) *o += std::to_string(k.col) + ",";
        *o += ";";
    }
    *o += "|";
    expr_sig(n->pred.get(), o);
    for (auto &pr : n->proj) { expr_sig(pr.first.get(), o); *o += pr.second + ","; }
    if (n->kind == NKind::Scan) {
        leaves->push_back(n->leaf);
        *o += pl->ir.leaves[(size_t)n->leaf].relation;
    }
    for (auto &c : n->in) node_sig(pl, c.get(), false, o, leaves);
    *o += "]";
}
void find_twins(flockgpu_plan *pl) {
    pl->twin_sig.assign((size_t)pl->ir.n_nodes, std::string());
    pl->twin_leaves.assign((size_t)pl->ir.n_nodes, std::vector<int>());
    std::map<std::string, std::vector<const Node *>> by_sig;
    std::vector<std::vector<int>> leaves((size_t)pl->ir.n_nodes);
    std::vector<const Node *> walk{pl->ir.root.get()};
    while (!walk.empty()) {
        const Node *n = walk.back();
        walk.pop_back();
        for (auto &c : n->in) walk.push_back(c.get());
        if (n->kind != NKind::Aggregate) continue;
        std::string sig;
        node_sig(pl, n, true, &sig, &leaves[(size_t)n->id]);
        by_sig[sig].push_back(n);
    }
    for (auto &kv : by_sig)
        if (kv.second.size() > 1)
            for (const Node *n : kv.second) {
                pl->twin_sig[(size_t)n->id] = kv.first;
                pl->twin_leaves[(size_t)n->id] = leaves[(size_t)n->id];
            }
}

int parse_and_build(flockgpu_ctx *ctx, const char *plan_json, size_t len, flockgpu_plan *pl, uint32_t flags = 0) {
    JParser jp{plan_json, plan_json + len, {}};
    JPtr root;
    if (!jp.parse(root) || root->kind != JValue::Obj)
        return fail(ctx, FLOCKGPU_ERR_PLAN, "plan: JSON error: %s", jp.err.empty() ? "not an object" : jp.err.c_str());
    if (!build_plan(root.get(), &pl->ir)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan: %s", pl->ir.why.c_str());
    pl->generic_only = (flags & FLOCKGPU_PLAN_GENERIC_ONLY) != 0;
    pl->fused.assign((size_t)pl->ir.n_nodes, FusedInfo{});
    recognise_fused(pl, pl->ir.root.get());
    pl->query = classify(pl);
    find_twins(pl);
    std::ostringstream os;
    describe(pl, pl->ir.root.get(), 0, os);
    pl->description = os.str();
    pl->leaves.resize(pl->ir.leaves.size());
    for (size_t i = 0; i < pl->leaves.size(); ++i) pl->leaves[i].cols.resize(pl->ir.leaves[i].schema.size());
    return FLOCKGPU_OK;
}

const char *format_of(const DevColumn &c) {
    if (c.is_ts) return "tsm:";
    switch (c.type) {
        case ColType::I32: return "i";
        case ColType::I64: return "l";
        case ColType::U64: return "L";
        case ColType::F64: return "g";
        default: return "u";
    }
}

// ------------------------------------------------------------------ execution
struct Exec {
    flockgpu_plan *pl;
    flockgpu_ctx *ctx;
    std::map<std::string, Table> memo;   // this execute's tables of the sub-trees that have twins (flockgpu_plan::twin_sig)
    // now() (valprog.hpp A-F8): the UTC wall clock in milliseconds, read once -- here, as the execute begins
    int64_t now_ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
    int fn_cols = 0;   // length columns written so far by this execute (octet_length / char_length: a buffer each, named by this count)
    int slice_bufs = 0;   // ... and the (begin, end) pairs of text slice calls (textslice.hpp)
    int cast_bufs = 0;    // ... and the Utf8 columns of numbers cast to text (numtext.hpp)
    std::map<std::string, DevColumn> cast_cols;   // the casts of the projection at hand by their text: identical casts are computed once (exec_project clears it)
    int parse_bufs = 0;   // ... and the numeric columns of text cast to numbers (textnum.hpp)
    std::map<std::string, DevColumn> parse_cols;   // the parses of the node at hand by their text: identical casts are parsed once (cleared with cast_cols)
    struct ParseFlag {
        const uint32_t *h_fail;   // pinned: the parse kernel stores a 1 where a value does not parse (textnum.hip)
        std::string what;
    };
    std::vector<ParseFlag> parse_pending;   // the cast_expr parses launched since the last wait of the evaluator

    // A relation the SQL scans twice (q5 and q7 read `bid` in both join inputs, q5_plan.fmt:6,13) has two MemoryExec leaves
    // but arrives as ONE source, which feed_data_sources hands to the first matching leaf (context.rs:273-300) -- the
    // second would stay empty.  An unfed leaf therefore reads the fed leaf that scans the same columns.
    int resolve_leaf(int leaf) const {
        if (pl->leaves[(size_t)leaf].rows > 0) return leaf;
        const Leaf &me = pl->ir.leaves[(size_t)leaf];
        for (size_t o = 0; o < pl->leaves.size(); ++o) {
            if ((int)o == leaf || pl->leaves[o].rows == 0) continue;
            const Leaf &other = pl->ir.leaves[o];
            bool ok = true;
            // (union.hpp A-U7) under COUNT(*) a branch of a union needs no column at all, and "every column it needs" holds of ANY fed leaf: an
            // input that was fed no rows would count another relation's.  In a plan with a union such a leaf reads only a leaf of its own field list.
            if (pl->ir.has_union && std::find(me.needed.begin(), me.needed.end(), 1) == me.needed.end()) {
                ok = other.schema.size() == me.schema.size();
                for (size_t c = 0; c < me.schema.size() && ok; ++c) ok = other.schema[c].name == me.schema[c].name && other.schema[c].type == me.schema[c].type;
            }
            for (size_t c = 0; c < me.schema.size() && ok; ++c) {
                if (!me.needed[c]) continue;
                ok = false;
                for (size_t d = 0; d < other.schema.size(); ++d)
                    if (other.schema[d].name == me.schema[c].name && other.schema[d].type == me.schema[c].type && other.needed[d]) ok = true;
            }
            if (ok) return (int)o;
        }
        return leaf;
    }
    int leaf_column(int leaf, int src_leaf, int col) const {  // column `col` of `leaf`, as an index into `src_leaf`
        if (leaf == src_leaf) return col;
        const Leaf &me = pl->ir.leaves[(size_t)leaf], &other = pl->ir.leaves[(size_t)src_leaf];
        for (size_t d = 0; d < other.schema.size(); ++d)
            if (other.schema[d].name == me.schema[(size_t)col].name) return (int)d;
        return -1;
    }

    int scan_table(const Node *n, Table *t) {
        const int src = resolve_leaf(n->leaf);
        const LeafData &ld = pl->leaves[(size_t)src];
        const Leaf &lf = pl->ir.leaves[(size_t)n->leaf];
        t->rows = ld.rows;
        t->cols.resize(n->schema.size());
        for (size_t i = 0; i < n->schema.size(); ++i) {
            TCol &tc = t->cols[i];
            tc.c.type = lf.schema[i].type;
            tc.c.is_ts = lf.schema[i].is_ts;
            tc.c.nullable = lf.schema[i].nullable;
            if (!lf.needed[i]) continue;
            tc.present = true;
            const DevBuf &b = ld.cols[(size_t)leaf_column(n->leaf, src, (int)i)];
            if (tc.c.type == ColType::UTF8 && !b.offsets) {  // never fed: an empty relation still has a one-entry offsets array
                void *p = nullptr;
                FG_TRY(arena_get(ctx, leaf_key(pl, n->leaf, (int)i, "empty").c_str(), 64, &p));
                FG_HIP(ctx, hipMemsetAsync(p, 0, 64, ctx->stream));
                tc.c.offsets = static_cast<int32_t *>(p);
                tc.c.values = static_cast<uint8_t *>(p) + 16;
            } else if (!b.values) {
                void *p = nullptr;
                FG_TRY(arena_get(ctx, leaf_key(pl, n->leaf, (int)i, "empty").c_str(), 64, &p));
                tc.c.values = p;
            } else {
                tc.c.values = b.values;
                tc.c.offsets = b.offsets;
                tc.c.bytes = b.bytes;
                if (b.valid && b.valid_rows > 0) {   // batches fed after the last one with NULLs: all valid
                    DevBuf &wb = pl->leaves[(size_t)src].cols[(size_t)leaf_column(n->leaf, src, (int)i)];
                    if (wb.valid_rows < ld.rows) {
                        FG_HIP(ctx, hipMemsetAsync(wb.valid + wb.valid_rows, 1, (size_t)(ld.rows - wb.valid_rows), ctx->stream));
                        wb.valid_rows = ld.rows;
                    }
                    tc.c.valid = b.valid;
                }
            }
        }
        return FLOCKGPU_OK;
    }
    // a fused pipeline reads plain NEXMark columns: a leaf column that carries validity sends its sub-tree to the generic operators
    bool leaf_has_validity(int leaf) const {
        if (leaf < 0) return false;
        for (auto &c : pl->leaves[(size_t)resolve_leaf(leaf)].cols)
            if (c.valid && c.valid_rows > 0) return true;
        return false;
    }

    // leaf column as a typed device pointer (fused entry points)
    template <typename T>
    const T *leaf_col(int leaf, int col) {
        if (col < 0) return nullptr;
        return static_cast<const T *>(pl->leaves[(size_t)leaf].cols[(size_t)col].values);
    }
    int leaf_utf8(int leaf, int col, flockgpu_utf8 *out) {
        const DevBuf &b = pl->leaves[(size_t)leaf].cols[(size_t)col];
        if (b.offsets) {
            *out = flockgpu_utf8{b.offsets, static_cast<const uint8_t *>(b.values)};
            return FLOCKGPU_OK;
        }
        void *p = nullptr;
        FG_TRY(arena_get(ctx, leaf_key(pl, leaf, col, "empty").c_str(), 64, &p));
        FG_HIP(ctx, hipMemsetAsync(p, 0, 64, ctx->stream));
        *out = flockgpu_utf8{static_cast<int32_t *>(p), static_cast<uint8_t *>(p) + 16};
        return FLOCKGPU_OK;
    }
    static flockgpu_windows whole(int64_t rows, int64_t (&off)[2], int32_t (&lo)[1], int32_t (&hi)[1]) {
        off[0] = 0; off[1] = rows; lo[0] = 0; hi[0] = 1;
        return flockgpu_windows{off, 1, lo, hi, 1};
    }
    static TCol dev_col(ColType t, const void *values, const int32_t *offsets = nullptr, int64_t bytes = 0, bool ts = false) {
        TCol c;
        c.present = true;
        c.c.type = t;
        c.c.is_ts = ts;
        c.c.values = values;
        c.c.offsets = offsets;
        c.c.bytes = bytes;
        return c;
    }
    // slots produced by a fused entry point -> the node's output columns
    void place(const Node *n, const FusedInfo &fi, const std::vector<TCol> &slots, int64_t rows, Table *t) {
        t->rows = rows;
        t->cols.assign(n->schema.size(), TCol{});
        for (size_t i = 0; i < n->schema.size(); ++i) {
            t->cols[i].c.type = n->schema[i].type;
            t->cols[i].c.is_ts = n->schema[i].is_ts;
            if (fi.out_map[i] < 0 || !n->required[i]) continue;
            t->cols[i] = slots[(size_t)fi.out_map[i]];
            t->cols[i].c.is_ts = n->schema[i].is_ts;
            t->cols[i].c.nullable = n->schema[i].nullable;
        }
    }

    int run_fused(const Node *n, const FusedInfo &fi, Table *t) {
        int64_t off_a[2], off_b[2];
        int32_t lo_a[1], hi_a[1], lo_b[1], hi_b[1];
        const LeafData &A = pl->leaves[(size_t)fi.leaf_a];
        switch (fi.kind) {
            case kQ2: {
                flockgpu_bid_cols bc{leaf_col<int32_t>(fi.leaf_a, fi.a_cols[0]), nullptr, leaf_col<int32_t>(fi.leaf_a, fi.a_cols[1]), nullptr, A.rows};
                flockgpu_windows w = whole(A.rows, off_a, lo_a, hi_a);
                flockgpu_q2_result r{};
                FG_TRY(flockgpu_q2_filter(ctx, &bc, &w, fi.lit, &r));
                place(n, fi, {dev_col(ColType::I32, r.auction), dev_col(ColType::I32, r.price)}, r.rows, t);
                return FLOCKGPU_OK;
            }
            case kPartialCount: {
                flockgpu_bid_cols bc{leaf_col<int32_t>(fi.leaf_a, fi.a_cols[0]), nullptr, nullptr, nullptr, A.rows};
                flockgpu_windows w = whole(A.rows, off_a, lo_a, hi_a);
                flockgpu_q5_partial_result r{};
                FG_TRY(flockgpu_q5_partial_counts(ctx, &bc, &w, &r));
                // node-owned copies: a second Partial COUNT of the same plan reuses the entry point's ctx-level buffers
                uint64_t *wide = nullptr;
                int32_t *keys = nullptr;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "cnt").c_str(), (size_t)r.rows + 2, &wide));
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "key").c_str(), (size_t)r.rows + 4, &keys));
                FG_TRY(widen_u32_to_u64(ctx, r.count, r.rows, wide));
                if (r.rows) FG_HIP(ctx, hipMemcpyAsync(keys, r.auction, sizeof(int32_t) * (size_t)r.rows, hipMemcpyDeviceToDevice, ctx->stream));
                place(n, fi, {dev_col(ColType::I32, keys), dev_col(ColType::U64, wide)}, r.rows, t);
                return FLOCKGPU_OK;
            }
            case kQ3: {
                const LeafData &B = pl->leaves[(size_t)fi.leaf_b];
                flockgpu_auction_cols ac{leaf_col<int32_t>(fi.leaf_a, fi.a_cols[0]), leaf_col<int32_t>(fi.leaf_a, fi.a_cols[1]),
                                         leaf_col<int32_t>(fi.leaf_a, fi.a_cols[2]), A.rows};
                flockgpu_person_cols pc{};
                pc.p_id = leaf_col<int32_t>(fi.leaf_b, fi.b_cols[0]);
                FG_TRY(leaf_utf8(fi.leaf_b, fi.b_cols[1], &pc.name));
                FG_TRY(leaf_utf8(fi.leaf_b, fi.b_cols[2], &pc.city));
                FG_TRY(leaf_utf8(fi.leaf_b, fi.b_cols[3], &pc.state));
                pc.rows = B.rows;
                flockgpu_windows aw = whole(A.rows, off_a, lo_a, hi_a), pw = whole(B.rows, off_b, lo_b, hi_b);
                std::vector<const char *> lits;
                for (auto &s : fi.strs) lits.push_back(s.c_str());
                flockgpu_q3_result r{};
                FG_TRY(flockgpu_q3_join(ctx, &ac, &aw, &pc, &pw, fi.lit, lits.data(), (int)lits.size(), &r));
                place(n, fi,
                      {dev_col(ColType::UTF8, r.name.data, r.name.offsets, r.name_bytes), dev_col(ColType::UTF8, r.city.data, r.city.offsets, r.city_bytes),
                       dev_col(ColType::UTF8, r.state.data, r.state.offsets, r.state_bytes), dev_col(ColType::I32, r.a_id)},
                      r.rows, t);
                return FLOCKGPU_OK;
            }
            case kQ5: {
                if (pl->ring_ppw && pl->ring_q5) {
                    // pane ring: every pane was counted once, when it was the newest (its Partial groups stay on the device); the window is
                    // the FinalPartitioned merge of the held panes' groups -> MAX -> join, i.e. q5.dag's second half over (auction, count) rows
                    FG_TRY(ring_q5_partial(pl));
                    int64_t total = 0;
                    for (int64_t g : pl->ring_groups) total += g;
                    flockgpu_windows w = whole(total, off_a, lo_a, hi_a);
                    flockgpu_q5_result r{};
                    API_CLOCK("ring.q5_weighted");
                    FG_TRY(flockgpu_q5_hot_items_weighted(ctx, pl->ring_auction, pl->ring_count, total, &w, &r));
                    place(n, fi, {dev_col(ColType::I32, r.auction), dev_col(ColType::U64, r.num)}, r.rows, t);
                    return FLOCKGPU_OK;
                }
                // both leaves scan the same relation; whichever was fed holds it (feed_data_sources gives it to the first match)
                const bool first = A.rows > 0 || pl->leaves[(size_t)fi.leaf_b].rows == 0;
                const int leaf = first ? fi.leaf_a : fi.leaf_b, col = first ? fi.a_cols[0] : fi.b_cols[0];
                const int64_t rows = pl->leaves[(size_t)leaf].rows;
                flockgpu_bid_cols bc{leaf_col<int32_t>(leaf, col), nullptr, nullptr, nullptr, rows};
                flockgpu_windows w = whole(rows, off_a, lo_a, hi_a);
                flockgpu_q5_result r{};
                API_CLOCK("q5_hot_items");
                FG_TRY(flockgpu_q5_hot_items(ctx, &bc, &w, &r));
                place(n, fi, {dev_col(ColType::I32, r.auction), dev_col(ColType::U64, r.num)}, r.rows, t);
                return FLOCKGPU_OK;
            }
            case kQ7: {
                const bool first = A.rows > 0 || pl->leaves[(size_t)fi.leaf_b].rows == 0;
                const int leaf = first ? fi.leaf_a : fi.leaf_b;
                const Leaf &lf = pl->ir.leaves[(size_t)leaf];
                auto by_name = [&](const char *nm) {
                    for (size_t i = 0; i < lf.schema.size(); ++i)
                        if (lf.schema[i].name == nm) return (int)i;
                    return -1;
                };
                const int64_t rows = pl->leaves[(size_t)leaf].rows;
                flockgpu_bid_cols bc{leaf_col<int32_t>(leaf, by_name("auction")), leaf_col<int32_t>(leaf, by_name("bidder")),
                                     leaf_col<int32_t>(leaf, by_name("price")), leaf_col<int64_t>(leaf, by_name("b_date_time")), rows};
                if (rows > 0 && (!bc.auction || !bc.bidder || !bc.price || !bc.b_date_time))
                    return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: the fed bid relation lacks a column of [auction, bidder, price, b_date_time]");
                flockgpu_windows w = whole(rows, off_a, lo_a, hi_a);
                flockgpu_q7_result r{};
                FG_TRY(flockgpu_q7_highest_bid(ctx, &bc, &w, &r));
                place(n, fi, {dev_col(ColType::I32, r.auction), dev_col(ColType::I32, r.bidder), dev_col(ColType::I32, r.price),
                              dev_col(ColType::I64, r.b_date_time, nullptr, 0, true)}, r.rows, t);
                return FLOCKGPU_OK;
            }
            case kQ13: {
                const LeafData &B = pl->leaves[(size_t)fi.leaf_b];
                flockgpu_bid_cols bc{leaf_col<int32_t>(fi.leaf_a, 0), leaf_col<int32_t>(fi.leaf_a, 1), leaf_col<int32_t>(fi.leaf_a, 2),
                                     leaf_col<int64_t>(fi.leaf_a, 3), A.rows};
                flockgpu_windows w = whole(A.rows, off_a, lo_a, hi_a);
                flockgpu_q13_result r{};
                FG_TRY(flockgpu_q13_side_join(ctx, &bc, &w, leaf_col<int32_t>(fi.leaf_b, 0), leaf_col<int32_t>(fi.leaf_b, 1), B.rows, &r));
                place(n, fi, {dev_col(ColType::I32, r.auction), dev_col(ColType::I32, r.bidder), dev_col(ColType::I32, r.price),
                              dev_col(ColType::I64, r.b_date_time, nullptr, 0, true), dev_col(ColType::I32, r.value)}, r.rows, t);
                return FLOCKGPU_OK;
            }
            case kQ8: {
                const LeafData &B = pl->leaves[(size_t)fi.leaf_b];
                flockgpu_person_cols pc{};
                pc.p_id = leaf_col<int32_t>(fi.leaf_a, fi.a_cols[0]);
                FG_TRY(leaf_utf8(fi.leaf_a, fi.a_cols[1], &pc.name));
                pc.rows = A.rows;
                flockgpu_auction_cols ac{nullptr, leaf_col<int32_t>(fi.leaf_b, fi.b_cols[0]), nullptr, B.rows};
                flockgpu_windows pw = whole(A.rows, off_a, lo_a, hi_a), aw = whole(B.rows, off_b, lo_b, hi_b);
                flockgpu_q8_result r{};
                FG_TRY(flockgpu_q8_join(ctx, &pc, &pw, &ac, &aw, &r));
                place(n, fi, {dev_col(ColType::I32, r.p_id), dev_col(ColType::UTF8, r.name.data, r.name.offsets, r.name_bytes)}, r.rows, t);
                return FLOCKGPU_OK;
            }
            case kQ9:
            case kQ4: {
                const bool q9 = fi.kind == kQ9;
                const LeafData &B = pl->leaves[(size_t)fi.leaf_b];
                if (B.rows == 0 && A.rows > 0 && q9)  // the bids went to the inner scan's leaf, which holds three of the four columns
                    return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: q9's bids were fed to the inner scan");
                flockgpu_auction_time_cols ac{leaf_col<int32_t>(fi.leaf_a, fi.a_cols[0]), leaf_col<int32_t>(fi.leaf_a, fi.a_cols[1]),
                                              leaf_col<int64_t>(fi.leaf_a, fi.a_cols[2]), leaf_col<int64_t>(fi.leaf_a, fi.a_cols[3]), A.rows};
                flockgpu_bid_cols bc{};
                if (q9) bc = flockgpu_bid_cols{leaf_col<int32_t>(fi.leaf_b, 0), leaf_col<int32_t>(fi.leaf_b, 1), leaf_col<int32_t>(fi.leaf_b, 2), leaf_col<int64_t>(fi.leaf_b, 3), B.rows};
                else bc = flockgpu_bid_cols{leaf_col<int32_t>(fi.leaf_b, fi.b_cols[0]), nullptr, leaf_col<int32_t>(fi.leaf_b, fi.b_cols[1]), leaf_col<int64_t>(fi.leaf_b, fi.b_cols[2]), B.rows};
                flockgpu_windows aw = whole(A.rows, off_a, lo_a, hi_a), bw = whole(B.rows, off_b, lo_b, hi_b);
                if (q9) {
                    flockgpu_q9_result r{};
                    FG_TRY(flockgpu_q9_winning_bids(ctx, &ac, &aw, &bc, &bw, &r));
                    place(n, fi, {dev_col(ColType::I32, r.auction), dev_col(ColType::I32, r.bidder), dev_col(ColType::I32, r.price),
                                  dev_col(ColType::I64, r.b_date_time, nullptr, 0, true)}, r.rows, t);
                } else {
                    flockgpu_q4_result r{};
                    FG_TRY(flockgpu_q4_avg_final_by_category(ctx, &ac, &aw, &bc, &bw, &r));
                    place(n, fi, {dev_col(ColType::I32, r.category), dev_col(ColType::F64, r.avg_final)}, r.rows, t);
                }
                return FLOCKGPU_OK;
            }
            case kYsb: {
                const LeafData &B = pl->leaves[(size_t)fi.leaf_b];
                flockgpu_ysb_event_cols ev{};
                FG_TRY(leaf_utf8(fi.leaf_a, fi.a_cols[0], &ev.ad_id));
                FG_TRY(leaf_utf8(fi.leaf_a, fi.a_cols[1], &ev.event_type));
                ev.rows = A.rows;
                flockgpu_ysb_campaign_cols cc{};
                FG_TRY(leaf_utf8(fi.leaf_b, fi.b_cols[0], &cc.c_ad_id));
                FG_TRY(leaf_utf8(fi.leaf_b, fi.b_cols[1], &cc.campaign_id));
                cc.rows = B.rows;
                flockgpu_windows w = whole(A.rows, off_a, lo_a, hi_a);
                flockgpu_ysb_result r{};
                FG_TRY(flockgpu_ysb_campaign_counts(ctx, &ev, &w, &cc, fi.strs[0].c_str(), &r));
                place(n, fi, {dev_col(ColType::UTF8, r.campaign_id.data, r.campaign_id.offsets, r.campaign_bytes), dev_col(ColType::U64, r.count)}, r.rows, t);
                return FLOCKGPU_OK;
            }
            default:
                return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: unknown fused pipeline");
        }
    }

    // ---- predicates
    static bool cmp_of(const std::string &op, CmpOp *out, bool flip) {
        static const struct { const char *n; CmpOp a, flipped; } t[] = {
            {"Eq", CmpOp::EQ, CmpOp::EQ}, {"NotEq", CmpOp::NE, CmpOp::NE}, {"Lt", CmpOp::LT, CmpOp::GT},
            {"LtEq", CmpOp::LE, CmpOp::GE}, {"Gt", CmpOp::GT, CmpOp::LT}, {"GtEq", CmpOp::GE, CmpOp::LE}};
        for (auto &e : t)
            if (op == e.n) { *out = flip ? e.flipped : e.a; return true; }
        return false;
    }
    // FilterExec's predicate -> the postfix program of pred.hpp (ONE kernel evaluates it per flag tile).  Leaves: a column against a
    // literal or another column (integers, Float64, Utf8 `=` / `<>`), `column % literal` against a literal, IS [NOT] NULL;
    // Utf8 LIKE / NOT LIKE / `<` `<=` `>` `>=` against a literal (a kernel of its own per leaf, strmatch.hpp: the program reads its words); a boolean
    // literal; IN lists become OR chains of `=` leaves; NOT / AND / OR combine in three-valued logic on the device.  AND / OR push
    // their deeper operand first (they commute), so the operand stack stays at log2(leaves) + 1.
    struct Operand {
        enum K { COL, INT, FLT, STR, MOD, NUL, BAD } k = BAD;
        const TCol *col = nullptr;
        int64_t i = 0;
        double f = 0;
        std::string s;
        int64_t modulus = 0;
        bool big = false;   // INT: a UInt64 literal above INT64_MAX (`i` is its bit pattern)
    };
    // `e` without the casts that change no value (and no NULL): to the operand's own type, Int32 -> Int64 / Float64, an integer literal to any
    // numeric type.  A cast that may truncate, overflow or -- TRY_CAST -- turn a value into NULL stays: the one-pass predicate program has
    // no leaf for it and the general evaluator (valprog.hpp) takes the predicate.
    const Expr *uncast_exact(const Expr *e, const Table &in) const {
        while (e && e->kind == EKind::Cast) {
            const Expr *x = e->l.get();
            const int from = val_type_of(x, in);
            const bool exact = from == (int)e->cast_to || (from == 0 && (e->cast_to == ColType::I64 || e->cast_to == ColType::F64)) || x->kind == EKind::LitI ||
                               (x->kind == EKind::LitF && e->cast_to == ColType::F64) || x->kind == EKind::LitNull;
            if (!exact) break;
            e = x;
        }
        return e;
    }
    Operand operand(const Expr *e, const Table &in) const {
        Operand o;
        bool neg = false;
        e = uncast_exact(e, in);
        while (e->kind == EKind::Neg) {   // -literal: folded here (a negated column is not taken)
            neg = !neg;
            e = uncast_exact(e->l.get(), in);
        }
        auto column = [&](const Expr *x) -> const TCol * {
            const TCol &c = in.cols[(size_t)x->col];
            return c.present || c.c.all_null ? &c : nullptr;
        };
        switch (e->kind) {
            case EKind::LitI:
                if (e->big_unsigned && neg) return o;   // -(a UInt64 beyond 2^63) is below every Int64: not a value any column type holds
                o.k = Operand::INT;
                o.i = neg ? (int64_t)(0 - (uint64_t)e->i) : e->i;
                o.big = e->big_unsigned;
                return o;
            case EKind::LitF: o.k = Operand::FLT; o.f = neg ? -e->f : e->f; return o;
            case EKind::LitS: if (!neg) { o.k = Operand::STR; o.s = e->s; } return o;
            case EKind::LitNull: o.k = Operand::NUL; return o;
            case EKind::Col:
                if (!neg && (o.col = column(e))) o.k = o.col->c.all_null ? Operand::NUL : Operand::COL;
                return o;
            case EKind::Bin:
                if (!neg && e->s == "Modulo") {
                    const Expr *c = uncast_exact(e->l.get(), in), *m = uncast_exact(e->r.get(), in);
                    if (c->kind == EKind::Col && m->kind == EKind::LitI && (o.col = column(c))) {
                        o.k = o.col->c.all_null ? Operand::NUL : Operand::MOD;
                        o.modulus = m->i;
                    }
                }
                return o;
            default: return o;
        }
    }
    static int pred_need(const Expr *e) {   // operand-stack slots the sub-tree needs when its deeper side goes first
        if (e->kind == EKind::Not) return pred_need(e->l.get());
        if (e->kind == EKind::Bin && (e->s == "And" || e->s == "Or")) {
            const int a = pred_need(e->l.get()), b = pred_need(e->r.get());
            return a == b ? a + 1 : std::max(a, b);
        }
        return e->kind == EKind::InList ? 2 : 1;
    }
    int pred_full() { return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: predicate beyond %d comparisons / %d columns / %d literal bytes", kPredMaxLeaves, kPredMaxCols, kPredLitPool); }
    int pred_const(PredBuilder &b, int v) {   // 0 FALSE, 1 TRUE, 2 NULL
        PredLeafDesc l{};
        l.kind = (uint8_t)PredLeafKind::Const;
        l.lit = v;
        return b.add_leaf(l) ? FLOCKGPU_OK : pred_full();
    }
    // `x op y` with the literal (if any) on the right
    int pred_compare(const std::string &opname, const Expr *le, const Expr *re, const Table &in, PredBuilder &b) {
        Operand l = operand(le, in), r = operand(re, in);
        bool flip = false;
        if (l.k == Operand::INT || l.k == Operand::FLT || l.k == Operand::STR) { std::swap(l, r); flip = true; }
        CmpOp op;
        if (!cmp_of(opname, &op, flip)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: operator '%s' in a predicate", opname.c_str());
        if (l.k == Operand::BAD || r.k == Operand::BAD) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: predicate shape is not supported");
        if (l.k == Operand::NUL || r.k == Operand::NUL) return pred_const(b, 2);   // a comparison with NULL is NULL
        PredLeafDesc d{};
        d.cmp = (uint8_t)op;
        auto is_int = [](const TCol *c) { return c->c.type == ColType::I32 || c->c.type == ColType::I64 || c->c.type == ColType::U64; };
        if (l.k == Operand::COL && r.k == Operand::COL) {
            const bool fa = l.col->c.type == ColType::F64, fb = r.col->c.type == ColType::F64;
            if (fa != fb || !(fa || (is_int(l.col) && is_int(r.col))) || ((l.col->c.type == ColType::U64) != (r.col->c.type == ColType::U64)))
                return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: column comparison needs two integer columns of one signedness, or two Float64 columns");
            d.kind = (uint8_t)(fa ? PredLeafKind::CmpF64Col : PredLeafKind::CmpIntCol);
            d.uns = l.col->c.type == ColType::U64;
            const int ia = b.add_col(l.col->c), ib = b.add_col(r.col->c);
            if (ia < 0 || ib < 0) return pred_full();
            d.a = (uint8_t)ia;
            d.b = (uint8_t)ib;
            return b.add_leaf(d) ? FLOCKGPU_OK : pred_full();
        }
        if (l.k != Operand::COL && l.k != Operand::MOD) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: a comparison of two literals");
        // from here on the right side is read as a literal: `a % 3 = b`, `a = b % 3`, `a % 2 = b % 2` have no one-pass leaf (the general
        // evaluator takes them) -- without this guard they would compare against r.i's default 0
        if (r.k != Operand::INT && r.k != Operand::FLT && r.k != Operand::STR)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: a column (or its remainder) against a non-literal has no one-pass leaf");
        const ColType ct = l.col->c.type;
        if (r.k == Operand::STR) {
            if (ct != ColType::UTF8 || l.k == Operand::MOD)
                return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: a Utf8 literal compares with a Utf8 column only");
            if (op != CmpOp::EQ && op != CmpOp::NE) {   // <, <=, >, >=: bytewise order, a kernel of its own (strmatch.hpp)
                StrPattern sp;
                std::string why;
                if (!strmatch_compile_cmp(r.s, (int)op, &sp, &why)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: Utf8 comparison with %s", why.c_str());
                return pred_words(l.col, sp, b);
            }
            d.kind = (uint8_t)PredLeafKind::Utf8Eq;
            d.negate = op == CmpOp::NE;
            d.lit_len = (int32_t)r.s.size();
            const int ia = b.add_col(l.col->c);
            if (ia < 0 || !b.add_literal(r.s, &d.lit_off)) return pred_full();
            d.a = (uint8_t)ia;
            return b.add_leaf(d) ? FLOCKGPU_OK : pred_full();
        }
        if (ct == ColType::UTF8) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: a Utf8 column against a number");
        if (ct == ColType::F64) {
            if (l.k == Operand::MOD) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: modulo of a Float64 column");
            d.kind = (uint8_t)PredLeafKind::CmpF64Lit;
            const double lit = r.k == Operand::FLT ? r.f : (double)r.i;
            std::memcpy(&d.lit, &lit, sizeof d.lit);
            const int ia = b.add_col(l.col->c);
            if (ia < 0) return pred_full();
            d.a = (uint8_t)ia;
            return b.add_leaf(d) ? FLOCKGPU_OK : pred_full();
        }
        // an integer column (or its remainder) against a number
        int64_t lit = r.i;
        if (r.k == Operand::FLT) {
            // CAST(int AS Float64) op f: exact as an integer comparison while the cast is (Int32 always; wider columns are not taken)
            if (ct != ColType::I32 || l.k == Operand::MOD || r.f != r.f) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: an Int64 column against a Float64 literal");
            const double fl = std::floor(r.f), ce = std::ceil(r.f);
            const bool whole = fl == r.f;
            if (!whole && (op == CmpOp::EQ || op == CmpOp::NE)) return pred_const_valid(b, l.col, op == CmpOp::NE);
            const double pick = (op == CmpOp::LT || op == CmpOp::GE) ? ce : fl;   // x < f <=> x < ceil f;  x <= f <=> x <= floor f;  x > f <=> x > floor f;  x >= f <=> x >= ceil f
            if (pick > 4e18) lit = INT64_MAX; else if (pick < -4e18) lit = INT64_MIN; else lit = (int64_t)pick;
        }
        if (r.k == Operand::INT && r.big && (ct != ColType::U64 || l.k == Operand::MOD))   // above every signed value (and every remainder)
            return pred_const_valid(b, l.col, op == CmpOp::NE || op == CmpOp::LT || op == CmpOp::LE);
        if (ct == ColType::U64 && !r.big && lit < 0)   // a negative literal is below every UInt64
            return pred_const_valid(b, l.col, op == CmpOp::NE || op == CmpOp::GT || op == CmpOp::GE);
        d.kind = (uint8_t)PredLeafKind::CmpIntLit;
        d.uns = ct == ColType::U64;
        if (l.k == Operand::MOD) {
            if (ct == ColType::U64) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: modulo needs a signed integer column");
            if (l.modulus == 0) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: modulo by zero (the reference raises a DataFusion error)");
            // x % -1 == 0 for every x (and INT64_MIN % -1 traps in hardware): the remainder by |m| has the same value
            const int64_t m = l.modulus == INT64_MIN ? l.modulus : (l.modulus < 0 ? -l.modulus : l.modulus);
            d.modulus = m;
            if (ct == ColType::I32 && m > 0 && m <= 0x7fffffffll) {
                d.mod_kind = 1;
                d.mod = umod32_make((uint32_t)m);
            } else {
                d.mod_kind = 2;
            }
        }
        if (ct == ColType::I32 && d.mod_kind != 2 && (lit > INT32_MAX || lit < INT32_MIN)) {
            // no Int32 (and no remainder by |m| < 2^31) reaches the literal: the comparison is the same for every non-NULL row
            const bool above = lit > INT32_MAX;
            const bool v = op == CmpOp::NE ? true : op == CmpOp::EQ ? false : (op == CmpOp::LT || op == CmpOp::LE) ? above : !above;
            return pred_const_valid(b, l.col, v);
        }
        d.lit = lit;
        const int ia = b.add_col(l.col->c);
        if (ia < 0) return pred_full();
        d.a = (uint8_t)ia;
        return b.add_leaf(d) ? FLOCKGPU_OK : pred_full();
    }
    // a comparison whose outcome is `v` for every row whose column is not NULL (NULL where it is): `col IS NOT NULL` when v, else NOT of it AND NULL...
    // expressed with the leaves at hand: v ? (col IS NOT NULL OR NULL) : (col IS NULL AND NULL)
    int pred_const_valid(PredBuilder &b, const TCol *col, bool v) {
        if (!col->c.valid) return pred_const(b, v ? 1 : 0);
        PredLeafDesc d{};
        d.kind = (uint8_t)PredLeafKind::IsNull;
        d.negate = v ? 1 : 0;
        const int ia = b.add_col(col->c);
        if (ia < 0) return pred_full();
        d.a = (uint8_t)ia;
        if (!b.add_leaf(d)) return pred_full();
        FG_TRY(pred_const(b, 2));
        return b.push(v ? PredOpKind::Or : PredOpKind::And) ? FLOCKGPU_OK : pred_full();
    }
    // A leaf whose TRUE bits a kernel of its own writes (strmatch.hip): launched here, read by the program's Words leaf
    const Node *words_node = nullptr;   // the filter being compiled (compile_filter)
    int words_used = 0;
    int pred_words(const TCol *col, const StrPattern &sp, PredBuilder &b) {
        if (!words_node) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: a string-match leaf outside a filter");
        uint32_t *words = nullptr;
        FG_TRY(strmatch_words(ctx, node_key(pl, words_node, "like", words_used++).c_str(), col->c, col_rows, sp, &words));
        PredLeafDesc d{};
        d.kind = (uint8_t)PredLeafKind::Words;
        d.lit = (int64_t)reinterpret_cast<uintptr_t>(words);
        const int ia = b.add_col(col->c);
        if (ia < 0) return pred_full();
        d.a = (uint8_t)ia;
        return b.add_leaf(d) ? FLOCKGPU_OK : pred_full();
    }
    int64_t col_rows = 0;   // rows of the filter's input
    int pred_like(const Expr *e, const Table &in, PredBuilder &b) {
        const Expr *c = uncast_exact(e->l.get(), in), *p = uncast_exact(e->r.get(), in);
        if (c->kind != EKind::Col || in.cols[(size_t)c->col].c.type != ColType::UTF8 || p->kind != EKind::LitS)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: LIKE takes a Utf8 column and a literal pattern");
        const TCol &col = in.cols[(size_t)c->col];
        if (col.c.all_null) return pred_const(b, 2);
        if (!col.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: predicate column was not materialised");
        StrPattern sp;
        std::string why;
        if (!strmatch_compile_like(p->s, &sp, &why)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: LIKE with %s", why.c_str());
        FG_TRY(pred_words(&col, sp, b));
        if (e->s == "NotLike" && !b.push(PredOpKind::Not)) return pred_full();
        return FLOCKGPU_OK;
    }
    int compile_pred(const Expr *e, const Table &in, PredBuilder &b) {
        switch (e->kind) {
            case EKind::LitB: return pred_const(b, e->i ? 1 : 0);
            case EKind::LitNull: return pred_const(b, 2);
            case EKind::Not:
                FG_TRY(compile_pred(e->l.get(), in, b));
                return b.push(PredOpKind::Not) ? FLOCKGPU_OK : pred_full();
            case EKind::IsNull:
            case EKind::IsNotNull: {
                const Expr *a = uncast_exact(e->l.get(), in);
                if (a->kind != EKind::Col) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: IS [NOT] NULL of something other than a column");
                const TCol &c = in.cols[(size_t)a->col];
                if (c.c.all_null) return pred_const(b, e->kind == EKind::IsNull ? 1 : 0);
                if (!c.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: predicate column was not materialised");
                if (!c.c.valid) return pred_const(b, e->kind == EKind::IsNull ? 0 : 1);
                PredLeafDesc d{};
                d.kind = (uint8_t)PredLeafKind::IsNull;
                d.negate = e->kind == EKind::IsNotNull;
                const int ia = b.add_col(c.c);
                if (ia < 0) return pred_full();
                d.a = (uint8_t)ia;
                return b.add_leaf(d) ? FLOCKGPU_OK : pred_full();
            }
            case EKind::InList: {   // x IN (a, b, ...) = (x = a) OR (x = b) OR ...; NOT IN = NOT of that (NULL when x is)
                for (size_t i = 0; i < e->list.size(); ++i) {
                    FG_TRY(pred_compare("Eq", e->l.get(), e->list[i].get(), in, b));
                    if (i > 0 && !b.push(PredOpKind::Or)) return pred_full();
                }
                if (e->negated && !b.push(PredOpKind::Not)) return pred_full();
                return FLOCKGPU_OK;
            }
            case EKind::Bin: {
                if (e->s == "And" || e->s == "Or") {
                    const Expr *first = e->l.get(), *second = e->r.get();
                    if (pred_need(second) > pred_need(first)) std::swap(first, second);
                    FG_TRY(compile_pred(first, in, b));
                    FG_TRY(compile_pred(second, in, b));
                    return b.push(e->s == "And" ? PredOpKind::And : PredOpKind::Or) ? FLOCKGPU_OK : pred_full();
                }
                if (e->s == "Like" || e->s == "NotLike") return pred_like(e, in, b);
                return pred_compare(e->s, e->l.get(), e->r.get(), in, b);
            }
            default:
                return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: predicate is not a comparison");
        }
    }

    // The Utf8 columns of one take share their row list: up to four of them go through ONE length pass, ONE scan, ONE host wait and
    // ONE emit launch (gather_utf8_multi_*) instead of a take -- and a wait -- per column.  A stage plan's operators materialise small
    // tables many times over (filter, join output, one take per repartition), and at that size the waits ARE the cost.
    // random_rows: the row list is in no order and names most rows (ORDER BY): fixed-width columns are taken as 16-byte records (gather_fixed_packed)
    int take_table(const Node *n, const Table &in, const std::vector<char> &required, const int32_t *rows, int64_t n_rows, int first_out, Table *out, bool random_rows = false) {
        std::vector<size_t> utf8;
        GatherCols batch;
        for (size_t i = 0; i < in.cols.size(); ++i) {
            TCol &o = out->cols[(size_t)first_out + i];
            o.c.type = in.cols[i].c.type;
            o.c.is_ts = in.cols[i].c.is_ts;
            o.c.nullable = in.cols[i].c.nullable;
            if (!required[(size_t)first_out + i] || !in.cols[i].present) continue;
            if (in.cols[i].c.type == ColType::UTF8) {
                utf8.push_back(i);
                continue;
            }
            o.present = true;
            o.subset_of = in.cols[i].subset_of ? in.cols[i].subset_of : in.cols[i].c.values;
            if (!in.cols[i].c.valid && n_rows > 0) {   // a fixed-width column without NULLs: one launch takes up to eight of them (gather_fixed_multi)
                void *pv = nullptr;
                FG_TRY(arena_get(ctx, (node_key(pl, n, "take", first_out + (int)i) + ".val").c_str(), (size_t)n_rows * col_width(in.cols[i].c.type) + 16, &pv));
                o.c = in.cols[i].c;
                o.c.values = pv;
                o.c.offsets = nullptr;
                o.c.bytes = 0;
                batch.src[batch.n] = in.cols[i].c.values;
                batch.out[batch.n] = pv;
                batch.width[batch.n] = (int32_t)col_width(in.cols[i].c.type);
                if (++batch.n == kGatherMulti) {
                    FG_TRY(gather_fixed_multi(ctx, batch, rows, n_rows));
                    batch.n = 0;
                }
                continue;
            }
            FG_TRY(take_column(ctx, node_key(pl, n, "take", first_out + (int)i).c_str(), in.cols[i].c, rows, n_rows, &o.c));
        }
        if (batch.n && random_rows) {   // groups of columns that fill a 16-byte record, in order
            int c0 = 0, grp = 0;
            while (c0 < batch.n) {
                GatherCols part;
                int bytes = 0;
                while (c0 < batch.n && part.n < 4 && bytes + batch.width[c0] <= 16) {
                    part.src[part.n] = batch.src[c0];
                    part.out[part.n] = batch.out[c0];
                    part.width[part.n] = batch.width[c0];
                    bytes += batch.width[c0];
                    ++part.n;
                    ++c0;
                }
                FG_TRY(gather_fixed_packed(ctx, node_key(pl, n, "takerec", first_out + grp++).c_str(), part, in.rows, rows, n_rows));
            }
        } else if (batch.n) {
            FG_TRY(gather_fixed_multi(ctx, batch, rows, n_rows));
        }
        for (size_t g0 = 0; g0 < utf8.size(); g0 += 4) {
            const int k = (int)std::min<size_t>(4, utf8.size() - g0);
            if (k == 1) {
                const size_t i = utf8[g0];
                TCol &o = out->cols[(size_t)first_out + i];
                FG_TRY(take_column(ctx, node_key(pl, n, "take", first_out + (int)i).c_str(), in.cols[i].c, rows, n_rows, &o.c));
                o.present = true;
                continue;
            }
            flockgpu_utf8 srcs[4], outs[4];
            int64_t nb[4];
            for (int j = 0; j < k; ++j) srcs[j] = flockgpu_utf8{in.cols[utf8[g0 + (size_t)j]].c.offsets, static_cast<const uint8_t *>(in.cols[utf8[g0 + (size_t)j]].c.values)};
            Utf8MultiGather g;
            FG_TRY(gather_utf8_multi_begin(ctx, node_key(pl, n, "mtake", first_out + (int)utf8[g0]).c_str(), srcs, k, rows, n_rows, &g));
            FG_TRY(gather_utf8_multi_wait(ctx, g));
            FG_TRY(gather_utf8_multi_finish(ctx, g, outs, nb));
            for (int j = 0; j < k; ++j) {
                const size_t i = utf8[g0 + (size_t)j];
                TCol &o = out->cols[(size_t)first_out + i];
                o.c.values = outs[j].data;
                o.c.offsets = outs[j].offsets;
                o.c.bytes = nb[j];
                o.present = true;
                if (in.cols[i].c.valid) {
                    uint8_t *v = nullptr;
                    FG_TRY(arena_get_t(ctx, node_key(pl, n, "mtakev", first_out + (int)i).c_str(), (size_t)std::max<int64_t>(n_rows, 0) + 16, &v));
                    FG_TRY(gather_u8(ctx, in.cols[i].c.valid, rows, n_rows, v));
                    o.c.valid = v;
                }
            }
        }
        return FLOCKGPU_OK;
    }

    // The statistics of a column that is NOT a leaf's cost a pass and a host wait on every execute (~20 us): worth it from several
    // thousand rows on, where the dense paths save more than that; below, the hash table answers (a stage plan's operators run on a
    // few thousand filtered rows, and at that size the waits ARE the cost -- DESIGN section 3a).  A leaf column's are cached.
    // rows of the leaf whose column lives at `values` (-1: no leaf's column)
    int64_t leaf_rows_of(const void *values) const {
        if (!values) return -1;
        for (auto &ld : pl->leaves)
            if (!ld.borrowed)
                for (auto &b : ld.cols)
                    if (b.values && b.values == values) return ld.rows;
        return -1;
    }
    bool stats_worth_it(const TCol &c, int64_t rows) const {
        if (rows >= (int64_t(1) << 13)) return true;   // (up to 4096 build rows the one-workgroup LDS join answers without any statistics)
        return leaf_rows_of(c.c.values) >= 0 || leaf_rows_of(c.subset_of) >= 0;
    }
    // (min, max) of an integer column for sizing the dense paths.  A LEAF column's are exact and remembered until the leaf changes
    // (flockgpu_plan::col_stats); a column taken FROM a leaf column (TCol::subset_of) gets the leaf's as bounds when the range they span is
    // still dense for its row count -- no pass, no wait --, its own exact ones otherwise.
    int leaf_col_stats(const void *values, ColType type, int64_t rows, int64_t *mn, int64_t *mx) {
        auto it = pl->col_stats.find(values);
        if (it != pl->col_stats.end() && it->second.rows == rows) {
            *mn = it->second.mn;
            *mx = it->second.mx;
            return FLOCKGPU_OK;
        }
        FG_TRY(column_minmax(ctx, plain_col(type, values), rows, mn, mx));
        pl->col_stats[values] = flockgpu_plan::ColStat{rows, *mn, *mx};
        return FLOCKGPU_OK;
    }
    int int_col_stats(const TCol &c, int64_t rows, int64_t *mn, int64_t *mx) {
        if (leaf_rows_of(c.c.values) >= 0) return leaf_col_stats(c.c.values, c.c.type, rows, mn, mx);
        const int64_t src_rows = c.subset_of && c.subset_of != c.c.values ? leaf_rows_of(c.subset_of) : -1;
        if (src_rows > 0 && rows > 0) {
            FG_TRY(leaf_col_stats(c.subset_of, c.c.type, src_rows, mn, mx));
            if (dense_range_ok(*mn, *mx, rows, c.c.type == ColType::U64)) return FLOCKGPU_OK;
        }
        return column_minmax(ctx, c.c, rows, mn, mx);
    }

    int key_i64(const Node *n, const TCol &c, int64_t rows, const char *what, int64_t **out) {
        if (!c.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: key column was not materialised");
        FG_TRY(arena_get_t(ctx, node_key(pl, n, what).c_str(), (size_t)rows + 2, out));
        return widen_to_i64(ctx, c.c, rows, *out);
    }

    // ---- the general expression evaluator (valprog.hpp): an expression tree -> its postfix program over the columns of `in`
    int val_unsupported(const char *what) { return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: %s", what); }
    int val_full() { return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: expression too large for one program (%d operators, %d columns, %d constants, depth %d)", kValMaxOps, kValMaxCols, kValMaxConsts, kValMaxStack); }
    // static type of `e` over the table's columns (expr_static_type's codes)
    int val_type_of(const Expr *e, const Table &in) const {
        std::vector<Field> sch(in.cols.size());
        for (size_t i = 0; i < in.cols.size(); ++i) sch[i].type = in.cols[i].c.type;
        return expr_static_type(e, sch);
    }
    // the type two operands meet in: the typed one's; two untyped literals take `hint`, else Float64 if one is written as one, else Int64
    int val_common_type(const Expr *a, const Expr *b, const Table &in, int hint) {
        const int ta = val_type_of(a, in), tb = val_type_of(b, in);
        if (ta == -2 || tb == -2 || ta == 4 || tb == 4) return -2;
        if (ta >= 0 && tb >= 0) return ta == tb ? ta : -2;
        if (ta >= 0) return ta;
        if (tb >= 0) return tb;
        if (hint >= 0 && hint <= 3) return hint;
        return (a->kind == EKind::LitF || b->kind == EKind::LitF) ? 3 : 1;
    }
    // pushes `e` (typed `want` where it is an untyped literal); *vt = what was pushed (0..3, 5)
    int val_compile(const Expr *e, const Table &in, ValBuilder &b, int want, int *vt, bool *may_null) {
        auto arith_op = [](const std::string &op) {
            return op == "Plus" ? ValOpKind::Add : op == "Minus" ? ValOpKind::Sub : op == "Multiply" ? ValOpKind::Mul : op == "Divide" ? ValOpKind::Div : ValOpKind::Mod;
        };
        auto cmp_op = [](const std::string &op, ValOpKind *k) {
            if (op == "Eq") *k = ValOpKind::Eq; else if (op == "NotEq") *k = ValOpKind::Ne; else if (op == "Lt") *k = ValOpKind::Lt;
            else if (op == "LtEq") *k = ValOpKind::Le; else if (op == "Gt") *k = ValOpKind::Gt; else if (op == "GtEq") *k = ValOpKind::Ge;
            else return false;
            return true;
        };
        switch (e->kind) {
            case EKind::Col: {
                const TCol &c = in.cols[(size_t)e->col];
                if (c.c.type == ColType::UTF8) return val_unsupported("a Utf8 column inside a computed expression");
                *vt = (int)c.c.type;
                if (c.c.all_null) {
                    *may_null = true;
                    return b.push(ValOpKind::Null, (ValType)*vt, 0) ? FLOCKGPU_OK : val_full();
                }
                if (!c.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: expression column was not materialised");
                *may_null = *may_null || c.c.valid != nullptr;
                return b.push(ValOpKind::Col, (ValType)*vt, 0, b.add_col(c.c)) ? FLOCKGPU_OK : val_full();
            }
            case EKind::LitI: case EKind::LitF: {
                int ty = val_type_of(e, in);
                if (ty < 0) ty = want >= 0 && want <= 3 ? want : (e->kind == EKind::LitF ? 3 : 1);
                uint64_t bits = 0;
                if (e->kind == EKind::LitF) {
                    if (ty != 3) return val_unsupported("a Float64 literal against an integer operand (the planner casts the column)");
                    std::memcpy(&bits, &e->f, 8);
                } else if (ty == 3) {
                    const double d = e->big_unsigned ? (double)(uint64_t)e->i : (double)e->i;
                    std::memcpy(&bits, &d, 8);
                } else {
                    if (e->big_unsigned && ty != 2) return val_unsupported("a UInt64 literal above 2^63 against a signed operand");
                    if (ty == 0 && (e->i < INT32_MIN || e->i > INT32_MAX)) return val_unsupported("a literal beyond the Int32 range of its operand");
                    if (ty == 2 && !e->big_unsigned && e->i < 0) return val_unsupported("a negative literal against a UInt64 operand");
                    bits = (uint64_t)e->i;
                }
                *vt = ty;
                return b.push(ValOpKind::Const, (ValType)ty, 0, b.add_const(bits)) ? FLOCKGPU_OK : val_full();
            }
            case EKind::LitB:
                *vt = 5;
                return b.push(ValOpKind::Const, ValType::BOOL, 0, b.add_const(e->i ? 1 : 0)) ? FLOCKGPU_OK : val_full();
            case EKind::LitNull:
                *vt = want >= 0 ? want : 1;
                *may_null = true;
                return b.push(ValOpKind::Null, (ValType)*vt, 0) ? FLOCKGPU_OK : val_full();
            case EKind::LitS:
                return val_unsupported("a Utf8 literal inside a computed expression");
            case EKind::Cast: {
                if (e->text_num) {   // text parsed to a number (textnum.hpp): a kernel of its own writes the column, the program reads it, its validity bytes with it
                    DevColumn d;
                    FG_TRY(parse_column(e, in, &d));
                    *vt = (int)e->cast_to;
                    *may_null = true;
                    if (d.all_null) return b.push(ValOpKind::Null, (ValType)*vt, 0) ? FLOCKGPU_OK : val_full();
                    return b.push(ValOpKind::Col, (ValType)*vt, 0, b.add_col(d)) ? FLOCKGPU_OK : val_full();
                }
                int from = -1;
                FG_TRY(val_compile(e->l.get(), in, b, -1, &from, may_null));
                if (from > 3 || (int)e->cast_to > 3) return val_unsupported("CAST between other than numeric types inside a computed expression");
                *vt = (int)e->cast_to;
                if (e->try_cast) *may_null = true;
                if (from == *vt) return FLOCKGPU_OK;
                return b.push(e->try_cast ? ValOpKind::TryCast : ValOpKind::Cast, (ValType)from, 1, 0, (ValType)*vt) ? FLOCKGPU_OK : val_full();
            }
            case EKind::Neg: {
                FG_TRY(val_compile(e->l.get(), in, b, want, vt, may_null));
                if (*vt == 2 || *vt > 3) return val_unsupported("unary minus of an unsigned or Boolean value");
                return b.push(ValOpKind::Neg, (ValType)*vt, 1) ? FLOCKGPU_OK : val_full();
            }
            case EKind::Not: {
                FG_TRY(val_compile(e->l.get(), in, b, 5, vt, may_null));
                if (*vt != 5) return val_unsupported("NOT of a value that is not Boolean");
                return b.push(ValOpKind::Not, ValType::BOOL, 1) ? FLOCKGPU_OK : val_full();
            }
            case EKind::IsNull: case EKind::IsNotNull: {
                int ty = -1;
                bool inner_null = false;
                FG_TRY(val_compile(e->l.get(), in, b, -1, &ty, &inner_null));
                *vt = 5;
                return b.push(e->kind == EKind::IsNull ? ValOpKind::IsNull : ValOpKind::IsNotNull, (ValType)ty, 1) ? FLOCKGPU_OK : val_full();
            }
            case EKind::InList: {   // (x = a) OR (x = b) OR ..., x evaluated once per item; NULL when x is
                for (size_t i = 0; i < e->list.size(); ++i) {
                    const int ty = val_common_type(e->l.get(), e->list[i].get(), in, -1);
                    if (ty < 0 || ty > 3) return val_unsupported("IN over operands without one numeric type");
                    int ta = -1, tb = -1;
                    FG_TRY(val_compile(e->l.get(), in, b, ty, &ta, may_null));
                    FG_TRY(val_compile(e->list[i].get(), in, b, ty, &tb, may_null));
                    if (ta != ty || tb != ty) return val_unsupported("IN over operands of different types");
                    if (!b.push(ValOpKind::Eq, (ValType)ty, 2)) return val_full();
                    if (i > 0 && !b.push(ValOpKind::Or, ValType::BOOL, 2)) return val_full();
                }
                if (e->negated && !b.push(ValOpKind::Not, ValType::BOOL, 1)) return val_full();
                *vt = 5;
                return FLOCKGPU_OK;
            }
            case EKind::Bin: {
                if (e->s == "And" || e->s == "Or") {
                    int ta = -1, tb = -1;
                    FG_TRY(val_compile(e->l.get(), in, b, 5, &ta, may_null));
                    FG_TRY(val_compile(e->r.get(), in, b, 5, &tb, may_null));
                    if (ta != 5 || tb != 5) return val_unsupported("AND / OR of values that are not Boolean");
                    *vt = 5;
                    return b.push(e->s == "And" ? ValOpKind::And : ValOpKind::Or, ValType::BOOL, 2) ? FLOCKGPU_OK : val_full();
                }
                ValOpKind ck;
                const bool is_cmp = cmp_op(e->s, &ck);
                if (!is_cmp && e->s != "Plus" && e->s != "Minus" && e->s != "Multiply" && e->s != "Divide" && e->s != "Modulo")
                    return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: binary operator '%s'", e->s.c_str());
                const int ty = val_common_type(e->l.get(), e->r.get(), in, is_cmp ? -1 : want);
                if (ty == 5 && is_cmp && (ck == ValOpKind::Eq || ck == ValOpKind::Ne)) {
                    // Boolean = Boolean
                } else if (ty < 0 || ty > 3) {
                    return val_unsupported("a binary operator over operands without one numeric type (the planner casts them to one)");
                }
                int ta = -1, tb = -1;
                FG_TRY(val_compile(e->l.get(), in, b, ty, &ta, may_null));
                FG_TRY(val_compile(e->r.get(), in, b, ty, &tb, may_null));
                if (ta != ty || tb != ty) return val_unsupported("a binary operator over operands of different types");
                *vt = is_cmp ? 5 : ty;
                return b.push(is_cmp ? ck : arith_op(e->s), (ValType)(ty == 5 ? 1 : ty), 2) ? FLOCKGPU_OK : val_full();
            }
            case EKind::Func: {
                if (e->fn == Fn::Now) {
                    *vt = 1;
                    return b.push(ValOpKind::Const, ValType::I64, 0, b.add_const((uint64_t)now_ms)) ? FLOCKGPU_OK : val_full();
                }
                if (e->fn == Fn::OctetLength || e->fn == Fn::CharLength) {   // a kernel of its own writes the lengths; the program reads them as an Int32 column
                    const Expr *c = e->list[0].get();
                    while (c->kind == EKind::Cast) c = c->l.get();
                    if (c->kind != EKind::Col || in.cols[(size_t)c->col].c.type != ColType::UTF8) return val_unsupported("a text length of something that is not a Utf8 column");
                    const TCol &col = in.cols[(size_t)c->col];
                    *vt = 0;
                    if (col.c.all_null) {
                        *may_null = true;
                        return b.push(ValOpKind::Null, ValType::I32, 0) ? FLOCKGPU_OK : val_full();
                    }
                    if (!col.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: expression column was not materialised");
                    int32_t *len = nullptr;
                    FG_TRY(utf8_lengths(ctx, node_key(pl, pl->ir.root.get(), "strlen", fn_cols++).c_str(), col.c, in.rows, e->fn == Fn::CharLength, &len));
                    DevColumn d;
                    d.type = ColType::I32;
                    d.values = len;
                    d.valid = col.c.valid;
                    *may_null = *may_null || d.valid != nullptr;
                    return b.push(ValOpKind::Col, ValType::I32, 0, b.add_col(d)) ? FLOCKGPU_OK : val_full();
                }
                if (fn_is_slice(e->fn)) return val_unsupported("a Utf8-valued function inside a computed expression");
                const bool math = fn_is_math(e->fn);
                int ta = -1;
                FG_TRY(val_compile(e->list[0].get(), in, b, math ? 3 : 1, &ta, may_null));
                if (ta != (math ? 3 : 1)) return val_unsupported("a scalar function over an argument of another type than it takes");
                const ValFn fn = math ? (ValFn)((int)ValFn::Abs + (int)e->fn)
                                      : (ValFn)((int)(e->fn == Fn::DateTrunc ? ValFn::TruncSecond : ValFn::PartSecond) + (int)e->i);
                *vt = math ? 3 : e->fn == Fn::DateTrunc ? 1 : 0;
                return b.push_func(fn, math ? ValType::F64 : ValType::I64) ? FLOCKGPU_OK : val_full();
            }
            case EKind::Case: {   // ELSE (or NULL), then from the LAST branch to the first: WHEN, THEN, Select -- the first TRUE WHEN wins
                int ty = val_type_of(e, in);
                if (ty == -1) ty = want >= 0 ? want : 1;
                if (ty < 0 || ty > 3) return val_unsupported("CASE without one numeric result type");
                int te = -1;
                if (e->r) {
                    FG_TRY(val_compile(e->r.get(), in, b, ty, &te, may_null));
                    if (te != ty) return val_unsupported("CASE branches of different types");
                } else {
                    *may_null = true;
                    if (!b.push(ValOpKind::Null, (ValType)ty, 0)) return val_full();
                }
                for (size_t i = e->list.size(); i >= 2; i -= 2) {
                    const Expr *w = e->list[i - 2].get(), *th = e->list[i - 1].get();
                    int tw = -1, tt = -1;
                    if (e->l) {   // CASE x WHEN v: x = v
                        const int tc = val_common_type(e->l.get(), w, in, -1);
                        if (tc < 0 || tc > 3) return val_unsupported("CASE operand and WHEN value without one numeric type");
                        int t1 = -1, t2 = -1;
                        FG_TRY(val_compile(e->l.get(), in, b, tc, &t1, may_null));
                        FG_TRY(val_compile(w, in, b, tc, &t2, may_null));
                        if (t1 != tc || t2 != tc) return val_unsupported("CASE operand and WHEN value of different types");
                        if (!b.push(ValOpKind::Eq, (ValType)tc, 2)) return val_full();
                    } else {
                        FG_TRY(val_compile(w, in, b, 5, &tw, may_null));
                        if (tw != 5) return val_unsupported("a WHEN that is not Boolean");
                    }
                    FG_TRY(val_compile(th, in, b, ty, &tt, may_null));
                    if (tt != ty) return val_unsupported("CASE branches of different types");
                    if (!b.push(ValOpKind::Select, (ValType)ty, 3)) return val_full();
                }
                *vt = ty;
                return FLOCKGPU_OK;
            }
        }
        return val_unsupported("an expression of an unknown kind");
    }

    // ---- text-valued expressions (textsel.hpp): `e` -> its sources in `tt` and its SELECTOR pushed onto `b` -- an Int32 value, the index of the source
    // the row takes; a NULL where the row has no value.  CASE is val_compile's CASE with the branches compiled here (nested CASE: nested Select).
    int text_full() { return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: more than %d distinct sources or %d bytes of literals in one Utf8-valued expression", kTextMaxSources, kTextMaxLiteralBytes); }
    int text_compile(const Expr *e, const Table &in, ValBuilder &b, TextTable &tt, bool *may_null) {
        auto source = [&](int idx) { return idx < 0 ? text_full() : b.push(ValOpKind::Const, ValType::I32, 0, b.add_const((uint64_t)idx)) ? FLOCKGPU_OK : val_full(); };
        auto null = [&]() {
            *may_null = true;
            return b.push(ValOpKind::Null, ValType::I32, 0) ? FLOCKGPU_OK : val_full();
        };
        switch (e->kind) {
            case EKind::LitS: return source(tt.add_literal(e->s));
            case EKind::LitNull: return null();
            case EKind::Cast: {
                if (e->cast_to != ColType::UTF8) return val_unsupported("CASE branches of different types");
                if (!e->num_text) return text_compile(e->l.get(), in, b, tt, may_null);
                DevColumn col;   // a number or timestamp made text (numtext.hpp): a column source
                FG_TRY(cast_column(e, in, &col));
                if (col.all_null) return null();
                return source(tt.add_column(col));
            }
            case EKind::Col: {
                const TCol &c = in.cols[(size_t)e->col];
                if (c.c.type != ColType::UTF8) return val_unsupported("CASE branches of different types");
                if (c.c.all_null) return null();
                if (!c.present || !c.c.offsets) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: expression column was not materialised");
                return source(tt.add_column(c.c));   // (its NULLs: the kernels read the column's validity bytes)
            }
            case EKind::Func: {   // a slice function (textslice.hpp): the chain of calls down to its column, innermost first, one launch each
                if (!fn_is_slice(e->fn)) return val_unsupported("CASE branches of different types");
                std::vector<const Expr *> chain;
                const Expr *c = e;
                while (c->kind == EKind::Func || (c->kind == EKind::Cast && !c->num_text)) {
                    if (c->kind == EKind::Func) {
                        if (!fn_is_slice(c->fn) || c->list.empty()) return val_unsupported("a text slice of something that is not a Utf8 column");
                        chain.push_back(c);
                        c = c->list[0].get();
                    } else {
                        c = c->l.get();
                    }
                }
                TCol col;
                if (c->kind == EKind::Cast) {   // the column under the slice is a number cast to Utf8 (numtext.hpp)
                    FG_TRY(cast_column(c, in, &col.c));
                    col.present = true;
                } else {
                    if (c->kind != EKind::Col || in.cols[(size_t)c->col].c.type != ColType::UTF8) return val_unsupported("a text slice of something that is not a Utf8 column");
                    col = in.cols[(size_t)c->col];
                }
                if (col.c.all_null) return null();
                if (!col.present || !col.c.offsets) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: expression column was not materialised");
                // (the key names the column by its position in `in`: identical calls of one expression are one source)
                const std::string key = slice_text(e, std::vector<std::string>());
                int idx = tt.find_slice(key);
                if (idx < 0) {
                    const int32_t *sb = nullptr, *se = nullptr;
                    for (size_t k = chain.size(); k-- > 0;) {
                        const Expr *f = chain[k];
                        SliceSpec spec;
                        spec.fn = slice_fn_of(f->fn);
                        spec.n = (int32_t)f->slice_n;
                        spec.arg = f->slice_arg;
                        int32_t *ob = nullptr, *oe = nullptr;
                        FG_TRY(text_slice(ctx, node_key(pl, pl->ir.root.get(), "slice", slice_bufs++).c_str(), col.c, in.rows, spec, sb, se, &ob, &oe));
                        sb = ob;
                        se = oe;
                    }
                    idx = tt.add_slice(col.c, sb, se, key);
                }
                return source(idx);   // (its NULLs: the column's validity bytes, as for a bare column)
            }
            case EKind::Case: {
                if (e->r) FG_TRY(text_compile(e->r.get(), in, b, tt, may_null));
                else FG_TRY(null());
                for (size_t i = e->list.size(); i >= 2; i -= 2) {
                    const Expr *w = e->list[i - 2].get(), *th = e->list[i - 1].get();
                    if (e->l) {   // CASE x WHEN v: x = v
                        const int tc = val_common_type(e->l.get(), w, in, -1);
                        if (tc < 0 || tc > 3) return val_unsupported("CASE operand and WHEN value without one numeric type");
                        int t1 = -1, t2 = -1;
                        FG_TRY(val_compile(e->l.get(), in, b, tc, &t1, may_null));
                        FG_TRY(val_compile(w, in, b, tc, &t2, may_null));
                        if (t1 != tc || t2 != tc) return val_unsupported("CASE operand and WHEN value of different types");
                        if (!b.push(ValOpKind::Eq, (ValType)tc, 2)) return val_full();
                    } else {
                        int tw = -1;
                        FG_TRY(val_compile(w, in, b, 5, &tw, may_null));
                        if (tw != 5) return val_unsupported("a WHEN that is not Boolean");
                    }
                    FG_TRY(text_compile(th, in, b, tt, may_null));
                    if (!b.push(ValOpKind::Select, ValType::I32, 3)) return val_full();
                }
                return FLOCKGPU_OK;
            }
            default: return val_unsupported("CASE branches of different types");
        }
    }
    // The casts of the node whose expressions are compiled next: `in` is its input table (a cast's key names columns by their position in it)
    void begin_casts(Table *in, const std::vector<Field> &schema) {
        cast_cols.clear();
        parse_cols.clear();
        for (size_t c = 0; c < in->cols.size() && c < schema.size(); ++c) in->cols[c].c.is_ts = schema[c].is_ts;   // (a cast of a timestamp to Utf8 reads it)
    }
    // After a wait of the evaluator on the stream: the failure words of the parse kernels queued in front of it (textnum.hpp A-TN3)
    int parse_check() {
        std::vector<ParseFlag> pending;
        pending.swap(parse_pending);
        for (auto &f : pending)
            if (__atomic_load_n(f.h_fail, __ATOMIC_ACQUIRE)) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: %s", f.what.c_str());
        return FLOCKGPU_OK;
    }
    // CAST(x AS Int32 / Int64 / UInt64 / Timestamp(ms)) of text (textnum.hpp) as a numeric column: x is a Utf8 column of `in` (read in place), a chain of
    // slice functions over one (the parse reads the slices' (begin, end) pairs), or any other text-valued expression, materialised first the way a
    // projected text column is.  Identical casts of one node are one column.
    int parse_column(const Expr *e, const Table &in, DevColumn *out) {
        const std::string key = expr_text(e, std::vector<std::string>());   // (columns by their position in `in`)
        auto hit = parse_cols.find(key);
        if (hit != parse_cols.end()) {
            *out = hit->second;
            return FLOCKGPU_OK;
        }
        const Node *root = pl->ir.root.get();
        const int slot = parse_bufs++;
        const TextNumKind kind = e->cast_ts ? TextNumKind::TS : e->cast_to == ColType::I32 ? TextNumKind::I32 : e->cast_to == ColType::U64 ? TextNumKind::U64 : TextNumKind::I64;
        // the operand: down the slice calls (and the casts of text to Utf8, which change nothing) to a column
        std::vector<const Expr *> chain;
        const Expr *c = e->l.get();
        while ((c->kind == EKind::Func && fn_is_slice(c->fn) && !c->list.empty()) || (c->kind == EKind::Cast && c->cast_to == ColType::UTF8 && !c->num_text)) {
            if (c->kind == EKind::Func) {
                chain.push_back(c);
                c = c->list[0].get();
            } else {
                c = c->l.get();
            }
        }
        DevColumn col;
        const int32_t *sb = nullptr, *se = nullptr;
        if (c->kind == EKind::Col && in.cols[(size_t)c->col].c.type == ColType::UTF8) {
            const TCol &tc = in.cols[(size_t)c->col];
            if (!tc.c.all_null && (!tc.present || !tc.c.offsets)) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: expression column was not materialised");
            col = tc.c;
            if (!col.all_null)
                for (size_t k = chain.size(); k-- > 0;) {   // innermost first, one launch each (text_compile's chain)
                    const Expr *f = chain[k];
                    SliceSpec spec;
                    spec.fn = slice_fn_of(f->fn);
                    spec.n = (int32_t)f->slice_n;
                    spec.arg = f->slice_arg;
                    int32_t *ob = nullptr, *oe = nullptr;
                    FG_TRY(text_slice(ctx, node_key(pl, root, "slice", slice_bufs++).c_str(), col, in.rows, spec, sb, se, &ob, &oe));
                    sb = ob;
                    se = oe;
                }
        } else {   // a text CASE, a number cast to Utf8, a slice of those: the column a projection of it would give
            TCol t;
            FG_TRY(text_value(e->l.get(), root, "tn", slot, in, &t));
            col = t.c;
        }
        if (col.all_null) {   // (every row NULL: nothing is launched)
            *out = DevColumn{};
            out->type = e->cast_to;
            out->is_ts = e->cast_ts;
            out->all_null = true;
        } else {
            const uint32_t *h_fail = nullptr;
            FG_TRY(text_to_num(ctx, node_key(pl, root, "textnum", slot).c_str(), col, in.rows, kind, e->try_cast, sb, se, out, &h_fail));
            static const char *types[] = {"Int32", "Int64", "UInt64", "Timestamp(ms)"};
            if (!e->try_cast && in.rows > 0)
                parse_pending.push_back({h_fail, std::string("cast_expr: a Utf8 value that is no ") + types[(int)kind] + " (CAST of Utf8 to " + types[(int)kind] + "; try_cast_expr gives NULL there)"});
        }
        parse_cols[key] = *out;
        return FLOCKGPU_OK;
    }
    // CAST(x AS Utf8) of a number or timestamp (numtext.hpp) as a Utf8 column: x is a column of `in`, or an expression the general evaluator computes
    // into a temporary column first.  Identical casts of one projection are one column.
    int cast_column(const Expr *e, const Table &in, DevColumn *out) {
        const std::string key = expr_text(e, std::vector<std::string>());   // (columns by their position in `in`)
        auto hit = cast_cols.find(key);
        if (hit != cast_cols.end()) {
            *out = hit->second;
            return FLOCKGPU_OK;
        }
        const Node *root = pl->ir.root.get();
        const int slot = cast_bufs++;
        const Expr *x = e->l.get();
        DevColumn src;
        if (x->kind == EKind::Col) {
            const TCol &c = in.cols[(size_t)x->col];
            if (!c.c.all_null && !c.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: expression column was not materialised");
            src = c.c;
        } else {
            ValBuilder vb;
            int vt = -1;
            bool may_null = false;
            FG_TRY(val_compile(x, in, vb, -1, &vt, &may_null));
            if (vt < 0 || vt > 2) return val_unsupported("CAST to Utf8 of a computed value that is not an integer or a Timestamp(ms)");
            void *vals = nullptr;
            uint8_t *vv = nullptr;
            FG_TRY(arena_get(ctx, node_key(pl, root, "castval", slot).c_str(), ((size_t)std::max<int64_t>(in.rows, 0) + 2) * 8, &vals));
            if (may_null) FG_TRY(arena_get_t(ctx, node_key(pl, root, "castvalv", slot).c_str(), (size_t)std::max<int64_t>(in.rows, 0) + 16, &vv));
            FG_TRY(valprog_to_column(ctx, node_key(pl, root, "castprog", slot).c_str(), vb.p, in.rows, (ColType)vt, vals, vv));
            FG_TRY(parse_check());
            src.type = (ColType)vt;
            src.is_ts = expr_is_ts(x);
            src.values = vals;
            src.valid = vv;
        }
        if (src.all_null) {
            *out = DevColumn{};
            out->type = ColType::UTF8;
            out->all_null = true;
        } else {
            FG_TRY(num_to_text(ctx, node_key(pl, root, "numtext", slot).c_str(), src, in.rows, e->try_cast, e->try_cast ? "try_cast_expr" : "cast_expr", out));
        }
        cast_cols[key] = *out;
        return FLOCKGPU_OK;
    }
    // Column i of projection `n` as text: the selector through the evaluator (none for a bare literal or column), then the length and emit passes
    int project_text(const Node *n, size_t i, const Table &in, TCol *o) { return text_value(n->proj[i].first.get(), n, "", (int)i, in, o); }
    // ... of any text-valued expression `e` over `in`; the buffers are named after node `n`, `pre` and `i`
    int text_value(const Expr *e, const Node *n, const char *pre, int i, const Table &in, TCol *o) {
        const std::string k_val = std::string(pre) + "val", k_valv = std::string(pre) + "valv", k_prog = std::string(pre) + "vprog", k_text = std::string(pre) + "text";
        ValBuilder vb;
        TextTable tt;
        bool may_null = false;
        FG_TRY(text_compile(e, in, vb, tt, &may_null));
        const int64_t rows = std::max<int64_t>(in.rows, 0);
        const int32_t *sel = nullptr;
        const uint8_t *sel_valid = nullptr;
        const bool bare = vb.p.n_ops == 1;   // one push: a literal, a column, a NULL
        if (bare && tt.s.k == 1 && tt.s.src[0].offsets && !tt.s.src[0].begin) {   // CAST(column AS Utf8): the column itself (a bare slice is one text_select)
            const Expr *c = e;
            while (c->kind == EKind::Cast && !c->num_text) c = c->l.get();
            if (c->kind == EKind::Cast) {   // a bare cast of a number: the column numtext.hip wrote
                DevColumn col;
                FG_TRY(cast_column(c, in, &col));
                *o = dev_col(ColType::UTF8, col.values, col.offsets, col.bytes);
                o->c.valid = col.valid;
                o->c.nullable = true;
                return FLOCKGPU_OK;
            }
            *o = in.cols[(size_t)c->col];
            o->c.nullable = true;
            return FLOCKGPU_OK;
        }
        if (!bare) {
            void *vals = nullptr;
            uint8_t *vv = nullptr;
            FG_TRY(arena_get(ctx, node_key(pl, n, k_val.c_str(), i).c_str(), ((size_t)rows + 2) * 8, &vals));
            if (may_null) FG_TRY(arena_get_t(ctx, node_key(pl, n, k_valv.c_str(), i).c_str(), (size_t)rows + 16, &vv));
            FG_TRY(valprog_to_column(ctx, node_key(pl, n, k_prog.c_str(), i).c_str(), vb.p, in.rows, ColType::I32, vals, vv));
            FG_TRY(parse_check());
            sel = static_cast<const int32_t *>(vals);
            sel_valid = vv;
        }
        DevColumn out;
        FG_TRY(text_select(ctx, node_key(pl, n, k_text.c_str(), i).c_str(), tt.s, sel, sel_valid, in.rows, &out));
        *o = dev_col(ColType::UTF8, out.values, out.offsets, out.bytes);
        o->c.valid = out.valid;
        o->c.nullable = true;
        return FLOCKGPU_OK;
    }

    // A filter's input table and its predicate compiled for it: the one-pass program of pred.hpp (*general = false, `b`), or -- a predicate that
    // program has no leaf for (arithmetic inside a comparison, CASE, casts of computed values) -- the general evaluator's (*general = true, `vb`),
    // which writes the same flag words + wave counts
    int compile_filter(const Node *n, Table *in, PredBuilder &b, ValBuilder &vb, bool *general) {
        FG_TRY(exec(n->in[0].get(), in));
        begin_casts(in, n->in[0]->schema);
        words_node = n;
        words_used = 0;
        col_rows = in->rows;
        const int rc = compile_pred(n->pred.get(), *in, b);
        words_node = nullptr;
        *general = rc == FLOCKGPU_ERR_UNSUPPORTED;
        if (!*general) return rc;
        int vt = -1;
        bool may_null = false;
        FG_TRY(val_compile(n->pred.get(), *in, vb, 5, &vt, &may_null));
        if (vt != 5) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: a filter predicate that is not Boolean");
        return FLOCKGPU_OK;
    }
    // FilterExec as a row selection: the input table and the rows of it the predicate keeps (input order) -- flags, scan, emit
    int filter_rows(const Node *n, Table *in, int32_t **rows, int64_t *n_out) {
        PredBuilder b;
        ValBuilder vb;
        bool general = false;
        FG_TRY(compile_filter(n, in, b, vb, &general));
        if (general) {
            FG_TRY(valprog_to_rows(ctx, node_key(pl, n, "vprog").c_str(), vb.p, in->rows, rows, n_out));
            return parse_check();
        }
        return pred_to_rows(ctx, node_key(pl, n, "sel").c_str(), b.p, in->rows, rows, n_out);
    }
    // The filter's predicate pass alone: flag words and wave counts over its INPUT table (pred.hpp pred_to_flags), for an ungrouped aggregate that
    // reads the input columns under them -- no scan, no emit, no take.
    int filter_flags(const Node *n, Table *in, const uint32_t **flags, const uint32_t **counts, int32_t *tiles) {
        PredBuilder b;
        ValBuilder vb;
        bool general = false;
        FG_TRY(compile_filter(n, in, b, vb, &general));
        if (general) {
            FG_TRY(valprog_to_flags(ctx, node_key(pl, n, "vprog").c_str(), vb.p, in->rows, flags, counts, tiles));
            return parse_check();
        }
        return pred_to_flags(ctx, node_key(pl, n, "sel").c_str(), b.p, in->rows, flags, counts, tiles);
    }

    // A FilterExec directly under a join (round 6): the filter's surviving rows as a ROW LIST over its input table -- nothing is taken yet.  The
    // join reads the key column through the list, and its result rows compose with it (via[pair row]), so the columns that only travel
    // through -- q3's three Utf8 columns of a person -- are gathered ONCE, at the join's output, instead of after the filter and again after
    // the join (a Utf8 take is three launches and a host wait).  `via` null: `base` is the table itself.
    struct Lazy {
        Table base;
        const int32_t *via = nullptr;
        int64_t rows = 0;
    };
    int exec_lazy(const Node *n, Lazy *z) {
        if (pl->fused[(size_t)n->id].kind == kNone) {
            if (n->kind == NKind::Repartition) return exec_lazy(n->in[0].get(), z);
            // a Semi / Anti join is a choice of rows of its left input, like a filter: nothing is taken until the consumer's output
            if (n->kind == NKind::Join && (n->join_type == JoinType::Semi || n->join_type == JoinType::Anti)) return exec_semi_lazy(n, z);
            if (n->kind == NKind::Filter) {
                int32_t *rows = nullptr;
                int64_t n_out = 0;
                FG_TRY(filter_rows(n, &z->base, &rows, &n_out));
                z->via = rows;
                z->rows = n_out;
                return FLOCKGPU_OK;
            }
            // a projection that only names columns of its input (the planner puts two of them between q8's DISTINCT and its join): the same rows,
            // the named columns
            if (n->kind == NKind::Project) {
                bool plain = !n->proj.empty();
                for (auto &pe : n->proj) plain = plain && pe.first->kind == EKind::Col;
                if (plain) {
                    Lazy below;
                    FG_TRY(exec_lazy(n->in[0].get(), &below));
                    z->base.rows = below.base.rows;
                    z->base.cols.assign(n->schema.size(), TCol{});
                    for (size_t i = 0; i < n->proj.size() && i < n->schema.size(); ++i) {
                        const size_t c = (size_t)n->proj[i].first->col;
                        if (c >= below.base.cols.size()) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: a projection names a column its input does not have");
                        z->base.cols[i] = below.base.cols[c];
                    }
                    z->via = below.via;
                    z->rows = below.rows;
                    return FLOCKGPU_OK;
                }
            }
            // DISTINCT (Int32, Utf8) -- q8's persons: `SELECT DISTINCT p_id, name` under the join -- is a choice of rows of its input: the input's
            // two columns and the chosen rows go up as they are, and the join takes the strings ONCE, for the rows that found a partner (the
            // aggregate's own take of both columns -- a length pass, a scan and an emit for the names -- was the second-largest item of q8 on the
            // generic operators)
            if (n->kind == NKind::Aggregate && pl->twin_sig[(size_t)n->id].empty()) {
                const Node *agg = n, *partial = nullptr;
                if (final_is_identity(n, &partial)) agg = partial;
                const Node *src = agg->in[0].get();
                if (pl->fused[(size_t)agg->id].kind == kNone && pl->twin_sig[(size_t)agg->id].empty() && agg->group.size() == 2 && agg->aggs.empty() &&
                    (size_t)agg->group[0] < src->schema.size() && (size_t)agg->group[1] < src->schema.size() &&
                    src->schema[(size_t)agg->group[0]].type == ColType::I32 && src->schema[(size_t)agg->group[1]].type == ColType::UTF8) {
                    Table in;
                    FG_TRY(exec(src, &in));
                    const TCol &k = in.cols[(size_t)agg->group[0]], &sc = in.cols[(size_t)agg->group[1]];
                    if (k.c.type != ColType::I32 || sc.c.type != ColType::UTF8 || !k.present || !sc.present)
                        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: two-column GROUP BY other than (Int32, Utf8)");
                    if (k.c.valid || sc.c.valid) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: DISTINCT over columns that hold NULLs");
                    int32_t *rows = nullptr;
                    int64_t n_out = 0;
                    FG_TRY(distinct_i32_utf8(ctx, node_key(pl, agg, "dist").c_str(), static_cast<const int32_t *>(k.c.values),
                                             flockgpu_utf8{sc.c.offsets, static_cast<const uint8_t *>(sc.c.values)}, in.rows, &rows, &n_out));
                    z->base.rows = in.rows;
                    z->base.cols = {k, sc};
                    for (size_t i = 0; i < 2 && i < n->schema.size(); ++i) {
                        z->base.cols[i].c.is_ts = n->schema[i].is_ts;
                        z->base.cols[i].c.nullable = n->schema[i].nullable;
                    }
                    z->via = rows;
                    z->rows = n_out;
                    return FLOCKGPU_OK;
                }
            }
        }
        FG_TRY(exec(n, &z->base));
        z->rows = z->base.rows;
        return FLOCKGPU_OK;
    }
    // out[i] = via[rows[i]]: rows of a side's row list -> rows of its base table (`via` null, or no rows: `rows` themselves)
    int compose_rows(const Node *n, const char *what, const int32_t *via, const int32_t *rows, int64_t count, const int32_t **out) {
        *out = rows;
        if (!via || count <= 0) return FLOCKGPU_OK;
        int32_t *composed = nullptr;
        FG_TRY(arena_get_t(ctx, node_key(pl, n, what).c_str(), (size_t)count + 4, &composed));
        FG_TRY(gather_i32(ctx, via, rows, count, composed));
        *out = composed;
        return FLOCKGPU_OK;
    }
    // `key` = column c of `z` as lazy_key returned it, with validity bytes: the rows whose key is not NULL become the side's row list (what a filter
    // on `key IS NOT NULL` would leave), and the key is taken through it.  One host wait (the row count).
    int drop_null_key_rows(const Node *n, Lazy *z, int c, const char *what, TCol *key) {
        PredBuilder b;
        PredLeafDesc d{};
        d.kind = (uint8_t)PredLeafKind::IsNull;
        d.negate = 1;
        const int ia = b.add_col(key->c);
        if (ia < 0) return pred_full();
        d.a = (uint8_t)ia;
        if (!b.add_leaf(d)) return pred_full();
        int32_t *rows = nullptr;
        int64_t n_out = 0;
        FG_TRY(pred_to_rows(ctx, node_key(pl, n, what).c_str(), b.p, z->rows, &rows, &n_out));
        FG_TRY(compose_rows(n, (std::string(what) + "v").c_str(), z->via, rows, n_out, &z->via));
        z->rows = n_out;
        const TCol &src = z->base.cols[(size_t)c];
        FG_TRY(take_column(ctx, node_key(pl, n, what, 2).c_str(), src.c, z->via, z->rows, &key->c));
        key->c.valid = nullptr;   // (every row of the list has a key)
        key->subset_of = src.subset_of ? src.subset_of : src.c.values;
        return FLOCKGPU_OK;
    }

    // column `c` of a lazy table as the join sees it: taken through the row list when there is one
    int lazy_key(const Node *n, const Lazy &z, int c, const char *what, int pair, TCol *out) {
        *out = z.base.cols[(size_t)c];
        if (!z.via || !out->present) return FLOCKGPU_OK;
        const TCol &src = z.base.cols[(size_t)c];
        FG_TRY(take_column(ctx, node_key(pl, n, what, pair).c_str(), src.c, z.via, z.rows, &out->c));
        out->subset_of = src.subset_of ? src.subset_of : src.c.values;
        return FLOCKGPU_OK;
    }
    // the join's result rows of one side: the pair rows composed with the side's row list, then ONE take of what the output needs
    int take_lazy(const Node *n, const Lazy &z, const int32_t *pair_rows, int64_t pairs, int first_out, const char *what, Table *t) {
        const int32_t *rows = nullptr;
        FG_TRY(compose_rows(n, what, z.via, pair_rows, pairs, &rows));
        return take_table(n, z.base, n->required, rows, pairs, first_out, t);
    }

    int exec(const Node *n, Table *t) {
        const FusedInfo &fi = pl->fused[(size_t)n->id];
        if (fi.kind != kNone && !leaf_has_validity(fi.leaf_a) && !leaf_has_validity(fi.leaf_b)) {
            const int rc = run_fused(n, fi, t);
            // q4 / q9's fused kernels need dense, increasing auction ids inside a batch (include/flockgpu.h); any other batch runs
            // on the generic operators below
            if (rc != FLOCKGPU_ERR_UNSUPPORTED || (fi.kind != kQ9 && fi.kind != kQ4)) return rc;
            *t = Table{};
        }
        switch (n->kind) {
            case NKind::Scan: return scan_table(n, t);
            case NKind::Repartition: return exec(n->in[0].get(), t);  // placement is unobservable in one process; the root case is handled by the caller
            case NKind::Filter: return exec_filter(n, t);
            case NKind::Project: return exec_project(n, t);
            case NKind::Sort: return exec_sort(n, -1, t);
            case NKind::Window: return exec_window(n, t);
            case NKind::Limit: return exec_limit(n, t);
            case NKind::Join: return n->join_type == JoinType::Cross ? exec_cross(n, t) : exec_join(n, t);
            case NKind::Union: return exec_union(n, t);
            case NKind::Aggregate: {
                const std::string &sig = pl->twin_sig[(size_t)n->id];
                if (sig.empty()) return exec_aggregate(n, t);
                // the sub-tree occurs more than once: one run per (signature, the leaves its scans read today); the twins get the table --
                // views of the first run's buffers, which nothing writes again before the next execute
                std::string key = sig;
                for (int leaf : pl->twin_leaves[(size_t)n->id]) key += "#" + std::to_string(resolve_leaf(leaf));
                auto it = memo.find(key);
                if (it != memo.end()) {
                    *t = it->second;
                    return FLOCKGPU_OK;
                }
                FG_TRY(exec_aggregate(n, t));
                memo[key] = *t;
                return FLOCKGPU_OK;
            }
        }
        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: unknown node");
    }

    int exec_filter(const Node *n, Table *t) {
        Table in;
        int32_t *rows = nullptr;
        int64_t n_out = 0;
        FG_TRY(filter_rows(n, &in, &rows, &n_out));
        t->rows = n_out;
        t->cols.assign(n->schema.size(), TCol{});
        return take_table(n, in, n->required, rows, n_out, 0, t);
    }

    int exec_project(const Node *n, Table *t) {
        Table in;
        FG_TRY(exec(n->in[0].get(), &in));
        begin_casts(&in, n->in[0]->schema);   // (the casts of THIS projection's input: numbers to Utf8, numtext.hpp; text to numbers, textnum.hpp)
        t->rows = in.rows;
        t->cols.assign(n->schema.size(), TCol{});
        for (size_t i = 0; i < n->proj.size(); ++i) {
            const Expr *e = n->proj[i].first.get();
            TCol &o = t->cols[i];
            o.c.type = n->schema[i].type;
            o.c.is_ts = n->schema[i].is_ts;
            if (!n->required[i]) continue;
            if (e->kind == EKind::Col) {
                o = in.cols[(size_t)e->col];
                continue;
            }
            if (n->schema[i].type == ColType::UTF8) {   // a text literal, CAST(column AS Utf8), CASE with text branches (textsel.hpp)
                FG_TRY(project_text(n, i, in, &o));
                continue;
            }
            // literal * CAST(Int32 column AS Float64): q1's currency conversion (planner.rs:90), one IEEE multiply
            const Expr *l = is_bin(e, "Multiply") ? e->l.get() : nullptr, *r = l ? e->r.get() : nullptr;
            if (l && l->kind != EKind::LitF && l->kind != EKind::LitI) std::swap(l, r);
            const Expr *c = r ? uncast(r) : nullptr;
            if (!l || n->schema[i].type != ColType::F64 || (l->kind != EKind::LitF && l->kind != EKind::LitI) || c->kind != EKind::Col ||
                in.cols[(size_t)c->col].c.type != ColType::I32 || !in.cols[(size_t)c->col].present) {
                // anything else: the general evaluator (valprog.hpp), one kernel per output column
                ValBuilder vb;
                int vt = -1;
                bool may_null = false;
                FG_TRY(val_compile(e, in, vb, (int)n->schema[i].type, &vt, &may_null));
                if (vt != (int)n->schema[i].type) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: a computed projection whose type is not its column's");
                void *vals = nullptr;
                uint8_t *vv = nullptr;
                FG_TRY(arena_get(ctx, node_key(pl, n, "val", (int)i).c_str(), ((size_t)std::max<int64_t>(in.rows, 0) + 2) * 8, &vals));
                if (may_null) FG_TRY(arena_get_t(ctx, node_key(pl, n, "valv", (int)i).c_str(), (size_t)std::max<int64_t>(in.rows, 0) + 16, &vv));
                FG_TRY(valprog_to_column(ctx, node_key(pl, n, "vprog", (int)i).c_str(), vb.p, in.rows, n->schema[i].type, vals, vv));
                FG_TRY(parse_check());
                o = dev_col(n->schema[i].type, vals, nullptr, 0, n->schema[i].is_ts);
                o.c.valid = vv;
                o.c.nullable = true;
                continue;
            }
            double *d = nullptr;
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "f64", (int)i).c_str(), (size_t)in.rows + 2, &d));
            flockgpu_bid_cols bc{nullptr, nullptr, static_cast<const int32_t *>(in.cols[(size_t)c->col].c.values), nullptr, in.rows};
            FG_TRY(flockgpu_q1_project(ctx, &bc, l->kind == EKind::LitF ? l->f : (double)l->i, d));
            o = dev_col(ColType::F64, d);
            o.c.valid = in.cols[(size_t)c->col].c.valid;   // literal * NULL is NULL
        }
        return FLOCKGPU_OK;
    }

    // WindowAggExec: the window columns first, then the input's (q6_plan.fmt: the WindowAggr schemas)
    int exec_window(const Node *n, Table *t) {
        Table in;
        FG_TRY(exec(n->in[0].get(), &in));
        const size_t nw = n->win.size();
        t->rows = in.rows;
        t->cols.assign(n->schema.size(), TCol{});
        auto key_of = [&](int col, DevColumn *out) -> int {
            const TCol &k = in.cols[(size_t)col];
            if (!k.present && !k.c.all_null) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: a window key column was not materialised");
            *out = k.c;
            if (k.c.all_null) { out->type = ColType::I32; out->values = nullptr; }   // every row NULL: one run as far as this key goes
            return FLOCKGPU_OK;
        };
        for (size_t w = 0; w < nw; ++w) {
            if (!n->win[w].row_number) continue;
            t->cols[w].c.type = ColType::U64;
            t->cols[w].c.nullable = true;
            if (!n->required[w]) continue;
            DevColumn keys[4];
            if (n->win[w].part.size() > 4) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: PARTITION BY more than four columns");
            for (size_t c = 0; c < n->win[w].part.size(); ++c) FG_TRY(key_of(n->win[w].part[c], &keys[c]));
            int nk = 0;
            DevColumn live[4];
            for (size_t c = 0; c < n->win[w].part.size(); ++c)
                if (keys[c].values) live[nk++] = keys[c];
            uint64_t *rank = nullptr;
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "rank", (int)w).c_str(), (size_t)std::max<int64_t>(in.rows, 0) + 2, &rank));
            FG_TRY(row_number_runs(ctx, node_key(pl, n, "rn", (int)w).c_str(), live, nk, in.rows, rank));
            t->cols[w] = dev_col(ColType::U64, rank);
            t->cols[w].c.nullable = true;
        }
        // aggregate columns: one window_aggregates call per distinct (PARTITION BY, ORDER BY) -- its keys are compared once
        std::vector<char> done(nw, 0);
        for (size_t w0 = 0; w0 < nw; ++w0) {
            if (n->win[w0].row_number || done[w0]) continue;
            const WinExpr &x0 = n->win[w0];
            auto same_keys = [&](const WinExpr &y) {
                if (y.row_number || y.part != x0.part || y.order.size() != x0.order.size()) return false;
                for (size_t k = 0; k < y.order.size(); ++k)
                    if (y.order[k].col != x0.order[k].col) return false;
                return true;
            };
            DevColumn live[2 * kMaxWindowKeys];   // (an all-NULL key splits nothing: left out)
            int np = 0, no = 0;
            for (int c : x0.part) {
                DevColumn k;
                FG_TRY(key_of(c, &k));
                if (k.values) live[np++] = k;
            }
            for (auto &o : x0.order) {
                DevColumn k;
                FG_TRY(key_of(o.col, &k));
                if (k.values) live[np + no++] = k;
            }
            std::vector<WinAgg> aggs;
            for (size_t w = w0; w < nw; ++w) {
                const WinExpr &x = n->win[w];
                if (!same_keys(x)) continue;
                done[w] = 1;
                const size_t width = x.type == ColType::I32 ? 4 : 8;
                TCol &oc = t->cols[w];
                oc.c.type = x.type;
                oc.c.is_ts = x.is_ts;
                oc.c.nullable = true;
                if (!n->required[w]) continue;
                WinAgg g;
                if (x.arg >= 0) {
                    const TCol &a = in.cols[(size_t)x.arg];
                    if (!a.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: a window argument column was not materialised");
                    if (!agg_takes(x.fn, a.c.type))
                        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: %s needs an integer column", agg_fn_name(x.fn));
                    g.values = a.c.values;
                    g.type = a.c.type;
                    g.valid = a.c.valid;
                }
                if (x.fn == AggFn::Avg) g.avg = true;
                else g.op = agg_op_for(x.fn, g.type);
                g.out_type = x.type;
                void *out = nullptr;
                FG_TRY(arena_get(ctx, node_key(pl, n, "wv", (int)w).c_str(), (size_t)std::max<int64_t>(in.rows, 0) * width + 64, &out));
                g.out = out;
                if (x.fn != AggFn::Count) FG_TRY(arena_get_t(ctx, node_key(pl, n, "wvv", (int)w).c_str(), (size_t)std::max<int64_t>(in.rows, 0) + 64, &g.out_valid));
                aggs.push_back(g);
                oc = dev_col(x.type, out, nullptr, 0, x.is_ts);
                oc.c.nullable = true;
                oc.c.valid = g.out_valid;
            }
            FG_TRY(window_aggregates(ctx, node_key(pl, n, "wa", (int)w0).c_str(), live, np, no, in.rows, aggs.data(), (int)aggs.size()));
        }
        for (size_t i = 0; i < in.cols.size(); ++i) t->cols[nw + i] = in.cols[i];
        return FLOCKGPU_OK;
    }

    // ORDER BY ... LIMIT n (context.rs:549-550): the order is computed for every row, only the first n are taken
    int exec_limit(const Node *n, Table *t) {
        const Node *c = n->in[0].get();
        if (c->kind == NKind::Sort && pl->fused[(size_t)c->id].kind == kNone) return exec_sort(c, n->limit, t);
        FG_TRY(exec(c, t));
        t->rows = std::min<int64_t>(t->rows, n->limit);   // (Utf8 columns keep their byte buffers: the first rows' offsets still hold)
        return FLOCKGPU_OK;
    }

    // ---- HashJoinExec.  The key columns of every pair as the join sees them -- taken through the sides' row lists (lazy_key) -- and what its paths
    // ask about them.
    struct JoinKeys {
        int np = 0;
        TCol l[kMaxKeyCols], r[kMaxKeyCols];
        bool l_null = false, r_null = false;     // per side: some key column holds nothing but NULLs (NULL keys never match: the side has no partner)
        bool l_valid = false, r_valid = false;   // per side: some key column carries validity bytes
        bool all_i32 = true;                     // every pair is Int32 = Int32
        bool any_text = false;                   // some pair is Utf8 = Utf8
        bool comparable = true;                  // (false: the second pair of an inner join on two -- it keeps a message of its own, exec_join)
    };
    int gather_join_keys(const Node *n, const Lazy &ZL, const Lazy &ZR, JoinKeys *k) {
        k->np = (int)n->on.size();
        if (k->np > kMaxKeyCols) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: a join on more than %d key pairs", kMaxKeyCols);
        for (int p = 0; p < k->np; ++p) {
            TCol &a = k->l[p], &b = k->r[p];
            FG_TRY(lazy_key(n, ZL, n->on[(size_t)p].l, "jkl", p, &a));
            FG_TRY(lazy_key(n, ZR, n->on[(size_t)p].r, "jkr", p, &b));
            if (!join_keys_comparable(a.c.type, b.c.type)) {   // (plan_ir.hpp: the rule Semi / Anti are refused by at create)
                // (an inner join on two pairs whose second cannot compare -- a Float64 column next to an integer pair -- keeps a message of its own)
                if (n->join_type != JoinType::Inner || k->np != 2 || p == 0 || k->any_text)
                    return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: join keys must be integer columns of one signedness, or two Utf8 columns");
                k->comparable = false;
            }
            if ((!a.present && !a.c.all_null) || (!b.present && !b.c.all_null)) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: key column was not materialised");
            k->l_null = k->l_null || a.c.all_null;
            k->r_null = k->r_null || b.c.all_null;
            k->l_valid = k->l_valid || a.c.valid;
            k->r_valid = k->r_valid || b.c.valid;
            k->all_i32 = k->all_i32 && a.c.type == ColType::I32 && b.c.type == ColType::I32;
            k->any_text = k->any_text || a.c.type == ColType::UTF8;
        }
        return FLOCKGPU_OK;
    }
    // two Int32 key columns compare as one 64-bit key
    int packed_pair_keys(const Node *n, const char *what, const TCol &a, const TCol &b, int64_t rows, int64_t **out) {
        FG_TRY(arena_get_t(ctx, node_key(pl, n, what).c_str(), (size_t)rows + 2, out));
        return pack_i32_pair(ctx, static_cast<const int32_t *>(a.c.values), static_cast<const int32_t *>(b.c.values), rows, *out);
    }
    // a column of plain values of one type: ids, dictionary codes
    static DevColumn plain_col(ColType t, const void *values) {
        DevColumn c;
        c.type = t;
        c.values = values;
        return c;
    }
    // the join's result: the pair rows of each side composed with the side's row list, then ONE take per side of what the output needs
    int emit_pairs(const Node *n, const Lazy &ZL, const Lazy &ZR, const int32_t *lrows, const int32_t *rrows, int64_t pairs, Table *t) {
        t->rows = pairs;
        FG_TRY(take_lazy(n, ZL, lrows, pairs, 0, "lzrl", t));
        return take_lazy(n, ZR, rrows, pairs, (int)ZL.base.cols.size(), "lzrr", t);
    }

    int exec_join(const Node *n, Table *t) {
        if (n->join_type != JoinType::Inner) {   // Semi / Anti: the kept left rows, then ONE take of the left columns somebody reads
            Lazy z;
            FG_TRY(exec_semi_lazy(n, &z));
            t->rows = z.rows;
            t->cols.assign(n->schema.size(), TCol{});
            if (!z.via) {   // (every row kept and no row list below: the left table itself)
                for (size_t i = 0; i < t->cols.size() && i < z.base.cols.size(); ++i) t->cols[i] = z.base.cols[i];
                return FLOCKGPU_OK;
            }
            return take_table(n, z.base, n->required, z.via, z.rows, 0, t);
        }
        Lazy ZL, ZR;
        FG_TRY(exec_lazy(n->in[0].get(), &ZL));
        FG_TRY(exec_lazy(n->in[1].get(), &ZR));
        t->cols.assign(n->schema.size(), TCol{});
        JoinKeys k;
        FG_TRY(gather_join_keys(n, ZL, ZR, &k));
        TCol &lk = k.l[0], &rk = k.r[0];
        int32_t *lrows = nullptr, *rrows = nullptr;
        int64_t pairs = 0;
        // Key pairs no path below takes -- more than two, or two that are not both Int32 without NULLs -- join on composite-key ids, NULLs allowed (a
        // NULL in any key column matches nothing): the smaller side's tuples get dense ids (relops.hpp key_codes), the other side looks its tuples
        // up among them, and the dense join pairs the ids -- the way the one-pair Utf8 join pairs dictionary codes.
        // (two pairs of which one cannot compare -- a Float64 column, Utf8 against an integer, signed against UInt64 -- keep today's path and message)
        if (k.np > 2 || (k.np == 2 && k.comparable && !(k.all_i32 && !k.l_valid && !k.r_valid))) {
            const int64_t nl = k.l_null ? 0 : ZL.rows, nr = k.r_null ? 0 : ZR.rows;
            if (nl > 0 && nr > 0) {
                DevColumn kl[kMaxKeyCols], kr[kMaxKeyCols];
                for (int p = 0; p < k.np; ++p) { kl[p] = k.l[p].c; kr[p] = k.r[p].c; }
                const bool build_right = nr < nl;   // (the ids go on the smaller side; which side is hashed is unobservable in the pair multiset)
                const int64_t nb = build_right ? nr : nl, npr = build_right ? nl : nr;
                int32_t *bg = nullptr, *pg = nullptr, *first = nullptr;
                int64_t groups = 0;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "kcb").c_str(), (size_t)nb + 4, &bg));
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "kcp").c_str(), (size_t)npr + 4, &pg));
                FG_TRY(key_codes(ctx, node_key(pl, n, "kc").c_str(), build_right ? kr : kl, k.np, nb, bg, &groups, &first, build_right ? kl : kr, npr, pg));
                FG_TRY(join_dense(ctx, node_key(pl, n, "join").c_str(), plain_col(ColType::I32, bg), nb, 0, groups - 1, plain_col(ColType::I32, pg), npr,
                                  build_right ? &rrows : &lrows, build_right ? &lrows : &rrows, &pairs));
            } else {   // an empty side: no pairs (the one-key join's answer to it)
                int64_t *none = nullptr;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "kc0").c_str(), 2, &none));
                FG_TRY(join_key64(ctx, node_key(pl, n, "join").c_str(), none, 0, none, 0, &lrows, &rrows, &pairs));
            }
            return emit_pairs(n, ZL, ZR, lrows, rrows, pairs, t);
        }
        const bool text_keys = k.np == 1 && k.any_text;
        // one key pair, a side whose key is a computed column with validity bytes -- an ungrouped aggregate's row (MAX over nothing is NULL), which
        // stays on the device: NULL keys never match, the side goes on as the row list of its valid keys
        if (k.np == 1 && k.l_valid && lk.present && !k.l_null) { FG_TRY(drop_null_key_rows(n, &ZL, n->on[0].l, "nnl", &lk)); k.l_valid = false; }
        if (k.np == 1 && k.r_valid && rk.present && !k.r_null) { FG_TRY(drop_null_key_rows(n, &ZR, n->on[0].r, "nnr", &rk)); k.r_valid = false; }
        const int64_t nl = k.l_null ? 0 : ZL.rows, nr = k.r_null ? 0 : ZR.rows;   // NULL keys never match
        // (NULLs in a LEAF's key column were left out at feed: inner-join keys are null-droppable.  A computed key column that carries
        // validity bytes -- a grouped MIN / MAX over nothing but NULLs joined on -- is not taken)
        if (k.l_valid || k.r_valid) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: join on a computed column that holds NULLs");
        // one integer key pair whose build side is dense: chain heads addressed by key - min (relops.hpp "dense integer keys").  The
        // table goes on the smaller side, as in join_key64 (which side is hashed is unobservable in the pair multiset).
        if (!text_keys && k.np == 1 && lk.present && rk.present && nl > 0 && nr > 0) {
            bool build_right = nl > 4 * nr && nl > 4096;
            // Which side is a primary key nothing says -- except the previous executes of this node: a build side that repeated keys
            // (auctions by seller in q3) while the other side never did (persons by id) hands the table to the other side when that one is
            // not much larger: unique build keys are probed as a filter, one pass and no chains (relops.hpp).  Each orientation keeps its own
            // finding (".dups" under its own name).
            const std::string nm_l = node_key(pl, n, "join"), nm_r = node_key(pl, n, "joinr");
            auto had_dups = [&](const std::string &nm) {
                auto it = ctx->host_i64.find(nm + ".dups");
                return it != ctx->host_i64.end() && !it->second.empty();
            };
            if (!build_right && had_dups(nm_l) && !had_dups(nm_r) && nr <= 4 * nl) build_right = true;
            else if (build_right && had_dups(nm_r) && !had_dups(nm_l) && nl <= 16 * nr) build_right = false;
            const TCol &bk = build_right ? rk : lk, &pk = build_right ? lk : rk;
            const int64_t nb = build_right ? nr : nl, np = build_right ? nl : nr;
            int64_t kmin = 0, kmax = 0;
            // (a join the one-workgroup LDS kernel takes is ONE launch and one wait -- the dense path's fill, build, count, scan and emit
            // are eight and a wait, whatever the statistics cost; anything larger is worth the pass, leaf or not)
            const bool look = !join_is_tiny(nl, nr);
            if (look) FG_TRY(int_col_stats(bk, nb, &kmin, &kmax));
            if (look && dense_range_ok(kmin, kmax, nb, bk.c.type == ColType::U64)) {
                FG_TRY(join_dense(ctx, (build_right ? nm_r : nm_l).c_str(), bk.c, nb, kmin, kmax, pk.c, np, build_right ? &rrows : &lrows, build_right ? &lrows : &rrows,
                                  &pairs));
                return emit_pairs(n, ZL, ZR, lrows, rrows, pairs, t);
            }
        }
        int64_t *kl = nullptr, *kr = nullptr;
        if (text_keys) {  // equal strings <-> equal dictionary codes (exact: full byte compare inside utf8_codes)
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "kl").c_str(), (size_t)nl + 2, &kl));
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "kr").c_str(), (size_t)nr + 2, &kr));
            FG_TRY(utf8_codes(ctx, node_key(pl, n, "codes").c_str(), lk.c, nl, kl, &rk.c, nr, kr));
            // the codes are row numbers of the left relation -- dense by construction, [0, nl) -- and a right string the left does not
            // hold gets a negative one: chain heads addressed by the code itself, no second hash table behind the dictionary's
            if (nl > 0 && nr > 0 && !join_is_tiny(nl, nr)) {
                FG_TRY(join_dense(ctx, node_key(pl, n, "join").c_str(), plain_col(ColType::I64, kl), nl, 0, nl - 1, plain_col(ColType::I64, kr), nr, &lrows, &rrows, &pairs));
                return emit_pairs(n, ZL, ZR, lrows, rrows, pairs, t);
            }
        } else if (k.np == 2) {  // two Int32 pairs compare as one 64-bit key
            if (!k.all_i32) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: a two-key join needs Int32 key columns");
            FG_TRY(packed_pair_keys(n, "kl", lk, k.l[1], nl, &kl));
            FG_TRY(packed_pair_keys(n, "kr", rk, k.r[1], nr, &kr));
        } else if (!join_is_tiny(nl, nr) && nl > 0 && nr > 0) {   // one integer key pair, not dense: the hashed table, keys read in their own types
            FG_TRY(join_hashed(ctx, node_key(pl, n, "join").c_str(), lk.c, nl, rk.c, nr, &lrows, &rrows, &pairs));
            return emit_pairs(n, ZL, ZR, lrows, rrows, pairs, t);
        } else {
            FG_TRY(key_i64(n, lk, nl, "kl", &kl));
            FG_TRY(key_i64(n, rk, nr, "kr", &kr));
        }
        FG_TRY(join_key64(ctx, node_key(pl, n, "join").c_str(), kl, nl, kr, nr, &lrows, &rrows, &pairs));
        return emit_pairs(n, ZL, ZR, lrows, rrows, pairs, t);
    }

    // CrossJoinExec (cross.hpp A-X1..6): L x R rows, pair (i, j) at row i * R + j, no pair lists -- left columns are repeats, right columns tiles,
    // produced for the columns somebody reads.  A side with a row list is taken once (L or R rows) and the result replicated.  A side of exactly one
    // row -- a global aggregate's -- leaves the other side's columns what they are (no kernel, no copy) and becomes fills.
    int exec_cross(const Node *n, Table *t) {
        Lazy Z[2];
        FG_TRY(exec_lazy(n->in[0].get(), &Z[0]));
        FG_TRY(exec_lazy(n->in[1].get(), &Z[1]));
        const int64_t L = std::max<int64_t>(Z[0].rows, 0), R = std::max<int64_t>(Z[1].rows, 0);
        const size_t nl = Z[0].base.cols.size();
        // (A-X6) the row count, before anything of the result exists
        int64_t rows = 0;
        if (!cross_rows_ok(L, R, &rows))
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: cross join (node %d) of %lld x %lld rows: more than 2^31 rows", n->id, (long long)L, (long long)R);
        t->rows = rows;
        t->cols.assign(n->schema.size(), TCol{});
        if (nl + Z[1].base.cols.size() != n->schema.size()) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: a cross join whose inputs are not its schema");
        // each side as a plain table of the columns somebody reads: its base, or ONE take through its row list (no rows at all: the empty take, A-X4)
        Table side;
        side.cols.assign(n->schema.size(), TCol{});
        for (int s = 0; s < 2; ++s) {
            const size_t first = s ? nl : 0;
            if (Z[s].via || rows == 0) {
                FG_TRY(take_table(n, Z[s].base, n->required, Z[s].via, rows == 0 ? 0 : Z[s].rows, (int)first, &side));
            } else {
                for (size_t i = 0; i < Z[s].base.cols.size(); ++i) {
                    side.cols[first + i] = Z[s].base.cols[i];
                    if (!n->required[first + i]) side.cols[first + i].present = false;
                }
            }
        }
        if (rows == 0) {
            *t = side;
            t->rows = 0;
            return FLOCKGPU_OK;
        }
        // (A-X6) every Utf8 column's bytes, before anything of the result exists
        for (size_t i = 0; i < side.cols.size(); ++i) {
            const TCol &c = side.cols[i];
            int64_t bytes = 0;
            if (c.present && c.c.type == ColType::UTF8 && !cross_bytes_ok(c.c.bytes, i < nl ? R : L, &bytes))
                return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: cross join (node %d) of %lld x %lld rows: Utf8 column '%s' exceeds 2^31 bytes", n->id, (long long)L,
                            (long long)R, n->schema[i].name.c_str());
        }
        for (size_t i = 0; i < side.cols.size(); ++i) {
            const TCol &c = side.cols[i];
            TCol &o = t->cols[i];
            o = c;
            if (!c.present) continue;
            const bool left = i < nl;
            // the other side is one row: this side's column IS the result's
            if ((left ? R : L) == 1) continue;
            o.subset_of = c.subset_of ? c.subset_of : c.c.values;   // (every value of the result is a value of the source)
            const std::string name = node_key(pl, n, "cross", (int)i);
            if (left) FG_TRY(cross_repeat(ctx, name.c_str(), c.c, L, R, &o.c));
            else FG_TRY(cross_tile(ctx, name.c_str(), c.c, R, L, &o.c));
        }
        return FLOCKGPU_OK;
    }

    // UnionExec (union.hpp A-U1..7): the inputs' rows one input after the other, for the columns somebody reads.  Every input arrives lazily: the
    // fixed-width columns and validity bytes of an input with a row list (a filter directly below) are read THROUGH the list by the union's kernels,
    // its Utf8 columns are taken once and concatenated.  The operator queues launches only; a wait is an input's own (its filter's count, its take).
    // Exactly one input with rows, and that one a plain table: its columns ARE the result -- no kernel, no copy.
    int exec_union(const Node *n, Table *t) {
        const size_t K = n->in.size(), C = n->schema.size();
        std::vector<Lazy> Z(K);
        std::vector<int64_t> rows(K, 0);
        for (size_t k = 0; k < K; ++k) {
            FG_TRY(exec_lazy(n->in[k].get(), &Z[k]));
            if (Z[k].base.cols.size() != C) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: union (node %d): input %zu is not of the union's schema", n->id, k);
            rows[k] = std::max<int64_t>(Z[k].rows, 0);
        }
        // (A-U6) the row count, before anything of the result exists
        int64_t total = 0;
        if (!union_rows_ok(rows.data(), (int)K, &total))
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: union (node %d) of %zu inputs: more than 2^31 rows", n->id, K);
        t->rows = total;
        t->cols.assign(C, TCol{});
        for (size_t i = 0; i < C; ++i) {
            t->cols[i].c.type = n->schema[i].type;
            t->cols[i].c.is_ts = n->schema[i].is_ts;
            t->cols[i].c.nullable = n->schema[i].nullable;
        }
        size_t with_rows = 0, only = 0;
        for (size_t k = 0; k < K; ++k)
            if (rows[k] > 0) { ++with_rows; only = k; }
        if (with_rows == 1) {
            const Lazy &z = Z[only];
            if (z.via) return take_table(n->in[only].get(), z.base, n->required, z.via, z.rows, 0, t);   // (the one take a filter's result costs anyway)
            for (size_t i = 0; i < C; ++i) {
                const bool nullable = t->cols[i].c.nullable;
                t->cols[i] = z.base.cols[i];
                t->cols[i].c.nullable = nullable;
                if (!n->required[i]) t->cols[i].present = false;
            }
            return FLOCKGPU_OK;
        }
        // the Utf8 columns of an input with a row list: ONE take of those somebody reads (the buffers are named after the input's node, which
        // materialises nothing itself on this path)
        std::vector<char> text(C, 0);
        bool any_text = false;
        for (size_t i = 0; i < C; ++i) {
            text[i] = n->required[i] && n->schema[i].type == ColType::UTF8;
            any_text = any_text || text[i];
        }
        std::vector<Table> taken(K);
        for (size_t k = 0; k < K && any_text; ++k) {
            if (!Z[k].via || rows[k] == 0) continue;
            taken[k].rows = rows[k];
            taken[k].cols.assign(C, TCol{});
            FG_TRY(take_table(n->in[k].get(), Z[k].base, text, Z[k].via, rows[k], 0, &taken[k]));
        }
        std::vector<std::vector<UnionInput>> ins(C);
        for (size_t i = 0; i < C; ++i) {
            if (!n->required[i]) continue;
            const bool utf8 = n->schema[i].type == ColType::UTF8;
            ins[i].resize(K);
            std::vector<int64_t> bytes(K, 0);
            for (size_t k = 0; k < K; ++k) {
                const bool was_taken = utf8 && Z[k].via && rows[k] > 0;
                const TCol &c = was_taken ? taken[k].cols[i] : Z[k].base.cols[i];
                if (rows[k] > 0 && !c.present && !c.c.all_null)
                    return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: union (node %d): column '%s' of input %zu was not materialised", n->id, n->schema[i].name.c_str(), k);
                if (c.c.type != n->schema[i].type)
                    return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: union (node %d): column '%s' of input %zu arrives in another type", n->id, n->schema[i].name.c_str(), k);
                ins[i][k].col = c.c;
                ins[i][k].via = utf8 ? nullptr : Z[k].via;
                ins[i][k].rows = rows[k];
                if (utf8 && rows[k] > 0 && !c.c.all_null) bytes[k] = c.c.bytes;
            }
            // (A-U6) every Utf8 column's bytes, before anything of the result exists
            int64_t sum = 0;
            if (utf8 && !union_bytes_ok(bytes.data(), (int)K, &sum))
                return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: union (node %d) of %zu inputs: Utf8 column '%s' exceeds 2^31 bytes", n->id, K, n->schema[i].name.c_str());
        }
        for (size_t i = 0; i < C; ++i) {
            if (!n->required[i]) continue;
            TCol &o = t->cols[i];
            const bool nullable = o.c.nullable;
            FG_TRY(union_column(ctx, node_key(pl, n, "union", (int)i).c_str(), ins[i].data(), (int)K, &o.c));
            o.c.is_ts = n->schema[i].is_ts;
            o.c.nullable = nullable || o.c.valid || o.c.all_null;
            o.present = true;
        }
        return FLOCKGPU_OK;
    }

    // HashJoinExec join_type Semi / Anti (relops.hpp A-S1..6) as a LAZY table: the left input's base table and the list of its rows that have
    // (Semi) / lack (Anti) a partner on the right.  The left side arrives lazily itself, its key columns are read through gather_join_keys, and the
    // kept rows compose with its row list -- no right-side take, no pair rows, no `.dups` bookkeeping.  Key shapes: one integer pair goes to
    // semi_rows (a bitmap when the right keys are dense, a hashed key set otherwise), two Int32 pairs as one packed 64-bit key to the same, one
    // Utf8 pair through utf8_codes, anything else -- more pairs, mixed types, NULLs in a multi-column key or on a computed right side -- through
    // key_codes; both already say "absent" per left row.  Empty and all-NULL sides are answered without a probe.
    int exec_semi_lazy(const Node *n, Lazy *z) {
        const bool anti = n->join_type == JoinType::Anti;
        Lazy ZL, ZR;
        FG_TRY(exec_lazy(n->in[0].get(), &ZL));
        FG_TRY(exec_lazy(n->in[1].get(), &ZR));
        const int64_t nl = ZL.rows, nr = ZR.rows;
        JoinKeys k;
        FG_TRY(gather_join_keys(n, ZL, ZR, &k));
        z->base = ZL.base;
        // (A-S4) nothing on the left, nothing that could match on the right, or nothing but NULL keys on the left: no probe
        if (nl <= 0 || nr <= 0 || k.r_null || k.l_null) {
            const bool keep_all = anti && nl > 0;
            z->rows = keep_all ? nl : 0;
            z->via = ZL.via;
            if (!keep_all) {   // (a row list of its own, so that "no rows" is not read as "the table itself")
                int32_t *none = nullptr;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "semi0").c_str(), 4, &none));
                z->via = none;
            }
            return FLOCKGPU_OK;
        }
        int32_t *rows = nullptr;
        int64_t n_out = 0;
        const std::string nm = node_key(pl, n, "semi");
        if (k.np == 1 && !k.any_text && !k.r_valid) {
            int64_t kmin = 0, kmax = 0;
            bool dense = false;
            // (a pair of sizes the one-workgroup kernel takes is ONE launch and one wait, whatever the statistics say; a leaf's statistics are cached)
            if (!semi_is_tiny(nl, nr)) {
                FG_TRY(int_col_stats(k.r[0], nr, &kmin, &kmax));
                dense = dense_range_ok(kmin, kmax, nr, k.r[0].c.type == ColType::U64);
            }
            FG_TRY(semi_rows(ctx, nm.c_str(), k.l[0].c, nl, k.r[0].c, nr, dense, kmin, kmax, anti, &rows, &n_out));
        } else if (k.np == 2 && k.all_i32 && !k.l_valid && !k.r_valid) {
            int64_t *kl = nullptr, *kr = nullptr;
            FG_TRY(packed_pair_keys(n, "kl", k.l[0], k.l[1], nl, &kl));
            FG_TRY(packed_pair_keys(n, "kr", k.r[0], k.r[1], nr, &kr));
            FG_TRY(semi_rows(ctx, nm.c_str(), plain_col(ColType::I64, kl), nl, plain_col(ColType::I64, kr), nr, false, 0, 0, anti, &rows, &n_out));
        } else if (k.np == 1 && k.any_text && !k.l_valid && !k.r_valid) {   // equal strings <-> a dictionary code of the right side (exact: full byte compare inside utf8_codes)
            int64_t *codes = nullptr;
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "kl").c_str(), (size_t)nl + 2, &codes));
            FG_TRY(utf8_codes(ctx, node_key(pl, n, "codes").c_str(), k.r[0].c, nr, nullptr, &k.l[0].c, nl, codes));
            FG_TRY(semi_rows_from_ids(ctx, nm.c_str(), codes, true, nl, anti, &rows, &n_out));
        } else {
            DevColumn kl[kMaxKeyCols], kr[kMaxKeyCols];
            for (int p = 0; p < k.np; ++p) { kl[p] = k.l[p].c; kr[p] = k.r[p].c; }
            int32_t *bg = nullptr, *pg = nullptr, *first = nullptr;
            int64_t groups = 0;
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "kcb").c_str(), (size_t)nr + 4, &bg));
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "kcp").c_str(), (size_t)nl + 4, &pg));
            FG_TRY(key_codes(ctx, node_key(pl, n, "kc").c_str(), kr, k.np, nr, bg, &groups, &first, kl, nl, pg));
            FG_TRY(semi_rows_from_ids(ctx, nm.c_str(), pg, false, nl, anti, &rows, &n_out));
        }
        z->rows = n_out;
        return compose_rows(n, "semiv", ZL.via, rows, n_out, &z->via);   // rows of the left input's own row list -> rows of its base table
    }

    // SortExec [+ GlobalLimitExec]: the stable order of relops.hpp's sort_rows, then one take of the columns somebody reads
    int exec_sort(const Node *n, int64_t limit, Table *t) {
        Table in;
        FG_TRY(exec(n->in[0].get(), &in));
        std::vector<SortKey> keys;
        for (auto &sc : n->sort_cols) {
            const TCol &c = in.cols[(size_t)sc.col];
            if (!c.present && !c.c.all_null) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: ORDER BY column was not materialised");
            keys.push_back(SortKey{c.c, sc.descending, sc.nulls_first});
        }
        int32_t *rows = nullptr;
        const int32_t *sorted_key = nullptr;   // the first key's column in sorted order, when the sort carried it (ORDER BY one ascending Int32 column)
        FG_TRY(sort_rows(ctx, node_key(pl, n, "sort").c_str(), keys.data(), (int)keys.size(), in.rows, &rows, &sorted_key));
        t->rows = limit >= 0 ? std::min<int64_t>(in.rows, limit) : in.rows;
        t->cols.assign(n->schema.size(), TCol{});
        std::vector<char> need = n->required;
        const size_t kc = n->sort_cols.empty() ? 0 : (size_t)n->sort_cols[0].col;
        if (sorted_key && kc < need.size() && need[kc]) need[kc] = 0;   // (no take of that column: 4 B / row at sorted-row positions, a quarter of sort.sql's takes)
        FG_TRY(take_table(n, in, need, rows, t->rows, 0, t, true));
        if (sorted_key && kc < need.size() && n->required[kc]) {
            TCol &o = t->cols[kc];
            o = dev_col(ColType::I32, const_cast<int32_t *>(sorted_key));
            o.c.is_ts = in.cols[kc].c.is_ts;
            o.c.nullable = in.cols[kc].c.nullable;
        }
        for (size_t i = 0; i < t->cols.size(); ++i) t->cols[i].c.all_null = in.cols[i].c.all_null;
        return FLOCKGPU_OK;
    }

    // Final / FinalPartitioned directly over the Partial of the SAME plan (only a repartition in between): the Partial saw the
    // whole input of this execute, so its output already holds every group exactly once and its state columns ARE the results
    // (COUNT / SUM / MAX / MIN states have the result's type; AVG's (count, sum) state does not).  The stage plans stage.rs cuts keep
    // Partial -> Hash repartition -> FinalPartitioned in one plan (q5.dag, q8.dag): a second hash pass over the groups for nothing.
    bool final_is_identity(const Node *n, const Node **partial) const {
        if (n->mode == AggMode::Partial || n->group.empty() || n->single_pass) return false;
        const Node *c = n->in[0].get();
        while (c->kind == NKind::Repartition) c = c->in[0].get();
        if (c->kind != NKind::Aggregate || c->mode != AggMode::Partial || c->group.size() != n->group.size() || c->aggs.size() != n->aggs.size() ||
            c->schema.size() != n->schema.size())
            return false;
        for (size_t i = 0; i < n->group.size(); ++i)
            if (n->group[i] != (int)i) return false;
        for (size_t a = 0; a < n->aggs.size(); ++a)
            if (n->aggs[a].fn != c->aggs[a].fn || n->aggs[a].fn == AggFn::Avg || n->aggs[a].arg != (int)(n->group.size() + a)) return false;
        for (size_t i = 0; i < n->schema.size(); ++i)
            if (c->schema[i].type != n->schema[i].type) return false;
        *partial = c;
        return true;
    }

    // these accumulators may take the dense (direct-address) table: integer ones over arguments without NULLs
    static bool specs_fit_dense(const AggSpec *specs, int n_specs) {
        for (int a = 0; a < n_specs; ++a)
            if (specs[a].valid || specs[a].op == AggOp::SUM_F64 || specs[a].op == AggOp::MAX_F64 || specs[a].op == AggOp::MIN_F64) return false;
        return true;
    }
    // GROUP BY on composite-key ids: gid in [0, G) in order of first appearance, then the dense GROUP BY over the ids (groups come out in id
    // order) where its accumulators allow, else the hashed one with its groups put back in id order.  g->first_row: the groups' first rows.
    int group_composite(const Node *n, const Table &in, const AggSpec *specs, int n_specs, GroupResultN *g, const int32_t **gid_out = nullptr) {
        const int nk = (int)n->group.size();
        DevColumn kc[kMaxKeyCols];
        for (int c = 0; c < nk; ++c) {
            const TCol &k = in.cols[(size_t)n->group[(size_t)c]];
            if (!k.present || k.c.all_null) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: GROUP BY a column that was not materialised");
            kc[c] = k.c;
        }
        int32_t *gid = nullptr, *first = nullptr;
        int64_t groups = 0;
        FG_TRY(arena_get_t(ctx, node_key(pl, n, "gid").c_str(), (size_t)in.rows + 4, &gid));
        FG_TRY(key_codes(ctx, node_key(pl, n, "kc").c_str(), kc, nk, in.rows, gid, &groups, &first, nullptr, 0, nullptr));
        *g = GroupResultN{};
        if (n_specs > 0) {
            if (groups > 0 && specs_fit_dense(specs, n_specs)) {
                FG_TRY(group_by_dense(ctx, node_key(pl, n, "grp").c_str(), plain_col(ColType::I32, gid), in.rows, 0, groups - 1, specs, n_specs, g));
            } else {
                int64_t *ids = nullptr;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "gid64").c_str(), (size_t)in.rows + 2, &ids));
                if (in.rows > 0) FG_TRY(widen_to_i64(ctx, plain_col(ColType::I32, gid), in.rows, ids));
                GroupResultN h;
                FG_TRY(group_by_key64_n(ctx, node_key(pl, n, "grp").c_str(), ids, in.rows, specs, n_specs, &h, nullptr));
                // (every id in [0, G) is one group: the accumulators go to position id)
                for (int a = 0; a < n_specs; ++a) {
                    FG_TRY(arena_get_t(ctx, node_key(pl, n, "gacc", a).c_str(), (size_t)groups + 2, &g->agg[a]));
                    FG_TRY(scatter_by_id_u64(ctx, h.keys, h.n_groups, h.agg[a], g->agg[a]));
                    if (h.agg_valid[a]) {
                        FG_TRY(arena_get_t(ctx, node_key(pl, n, "gaccv", a).c_str(), (size_t)groups + 16, &g->agg_valid[a]));
                        FG_TRY(scatter_by_id_u8(ctx, h.keys, h.n_groups, h.agg_valid[a], g->agg_valid[a]));
                    }
                }
            }
        }
        g->n_groups = groups;
        g->first_row = first;
        if (gid_out) *gid_out = gid;
        return FLOCKGPU_OK;
    }

    // The FilterExec an ungrouped aggregate sits on, through repartitions and projections that only name columns; map[c] = the filter's column
    // behind column c of `src`.  Null: something else is below (it is materialised as ever).
    const Node *filter_below(const Node *src, std::vector<int> *map) const {
        std::vector<int> m(src->schema.size());
        for (size_t i = 0; i < m.size(); ++i) m[i] = (int)i;
        for (const Node *c = src;;) {
            // (a filter over bids the q2 pipeline would run -- and materialise -- is read under its flags like any other)
            const Fused fk = pl->fused[(size_t)c->id].kind;
            if (fk != kNone && !(fk == kQ2 && c->kind == NKind::Filter)) return nullptr;
            if (c->kind == NKind::Repartition) {
                c = c->in[0].get();
            } else if (c->kind == NKind::Project) {
                for (auto &pe : c->proj)
                    if (pe.first->kind != EKind::Col) return nullptr;
                for (int &x : m) {
                    if ((size_t)x >= c->proj.size()) return nullptr;
                    x = c->proj[(size_t)x].first->col;
                }
                c = c->in[0].get();
            } else if (c->kind == NKind::Filter) {
                for (int x : m)
                    if (x < 0 || (size_t)x >= c->schema.size()) return nullptr;
                *map = m;
                return c;
            } else {
                return nullptr;
            }
        }
    }

    // ---- HashAggregateExec.  lower_aggregates restates a node's aggregates ONCE, as accumulators and as result columns described from them (WideOut,
    // groupwide.hpp).  Three back-ends run the two lists: the ungrouped streaming pass (reduce.hpp), the tables of relops.hpp (at most kMaxGroupAggs
    // accumulators) and the one pass over group ids of groupwide.hpp (up to kMaxWideAggs).  A new aggregate function is added in the lowering, with a
    // kernel op where it needs one.
    struct AggAcc {
        AggOp op = AggOp::COUNT;
        int col = -1;             // input column of the argument (-1: COUNT(*)): an index -- each back-end resolves pointers under its own rule
        bool with_valid = true;   // NULL arguments reach no accumulator (false: a Final's sums of states, which read every state row)
    };
    struct AggLowering {
        AggAcc accs[kMaxWideAggs];
        int n_accs = 0;
        std::vector<WideOut> outs;   // one per column of the node's schema behind the keys
    };
    // `grouped` stands for the differences between the back-ends that the node's result or refusal depends on; each is marked "(back-ends)" below.
    // Every refusal of an aggregate is made here, before a table runs, one aggregate after the other.  A node that earns two refusals at once can so
    // name another of them than it did while the checks were spread out: "into a column of another kind" used to follow the grouped tables (and the
    // refusals of number_groups: pair key types, a Float64 key), and to precede, aggregate by aggregate, the ungrouped pass's "more than %d argument
    // columns", which now follows the whole list.
    int lower_aggregates(const Node *n, const Table &in, bool grouped, AggLowering *L) {
        const bool is_final = n->mode != AggMode::Partial && !n->single_pass;
        // (back-ends) an argument nobody materialised because it holds nothing but NULLs: the ungrouped pass takes it (no program column, every
        // result over it NULL or 0), the grouped tables read pointers and refuse it
        auto readable = [&](const TCol &v) { return v.present || (!grouped && v.c.all_null); };
        auto need = [&](const TCol *v, AggFn as, const char *what) -> int {
            if (!v || !agg_takes(as, v->c.type) || !readable(*v)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: %s needs an integer column", what);
            return FLOCKGPU_OK;
        };
        auto acc = [&](AggOp op, int col, bool with_valid) {
            L->accs[L->n_accs] = AggAcc{op, col, with_valid};
            return L->n_accs++;
        };
        for (size_t ai = 0; ai < n->aggs.size(); ++ai) {
            const Agg &a = n->aggs[ai];
            // (the ungrouped pass has refused more than kReduceMaxSlots before it comes here)
            if (L->n_accs + ir::agg_accumulators(a.fn) > kMaxWideAggs) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: more than %d accumulators in one GROUP BY", kMaxWideAggs);
            const TCol *v = a.arg >= 0 && (size_t)a.arg < in.cols.size() ? &in.cols[(size_t)a.arg] : nullptr;
            const size_t oc = n->group.size() + L->outs.size();
            const ColType want = oc < n->schema.size() ? n->schema[oc].type : ColType::U64;
            if (a.fn == AggFn::CountDistinct) {   // no accumulator: a table of its own, behind the others on the stream
                if (!v || !agg_takes(a.fn, v->c.type) || !(v->present || v->c.all_null))
                    return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: distinct_count needs an integer or Utf8 column");
                L->outs.push_back(WideOut{WideOutKind::DistinctCount, (int)ai, -1, ColType::U64, 0});
            } else if (a.fn == AggFn::Count && is_final) {   // the sum of the count states, every state row read: over no state row it is 0, not NULL
                FG_TRY(need(v, AggFn::Sum, "the COUNT state"));
                L->outs.push_back(WideOut{WideOutKind::Value, acc(AggOp::SUM_INT, a.arg, false), -1, want, 0});
            } else if (a.fn == AggFn::Count) {   // COUNT(*) / COUNT(UInt8(1)) counts rows, COUNT(col) the rows whose col is not NULL: only its validity is read
                // (back-ends) grouped, any column will do; the ungrouped pass streams fixed-width columns -- no Utf8 -- and wants the column
                // materialised where it has validity to read
                if (!grouped && a.arg >= 0) {
                    if (!v || v->c.type == ColType::UTF8) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: count needs an integer column");
                    if (v->c.all_null || v->c.valid) FG_TRY(need(v, AggFn::Count, "count"));
                }
                L->outs.push_back(WideOut{WideOutKind::Value, acc(AggOp::COUNT, a.arg, true), -1, want, 0});
            } else if (a.fn != AggFn::Avg) {   // SUM of an integer column; MIN / MAX of an integer or a Float64 one
                FG_TRY(need(v, a.fn, agg_fn_name(a.fn)));
                const ColType at = v->c.type;
                // ... into a column of another kind.  (back-ends) The grouped finish narrows a 64-bit accumulator into an Int32 column and checks SUM
                // as well; the ungrouped fold writes 64-bit words, so MIN / MAX there keep Int32 to Int32, and SUM goes unchecked
                const bool other = want == ColType::UTF8 || (want == ColType::F64) != (at == ColType::F64) || (!grouped && (want == ColType::I32) != (at == ColType::I32));
                if (other && (grouped || agg_is_minmax(a.fn)))
                    return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: %s of a column into a column of another kind", agg_fn_name(a.fn));
                // MIN / MAX / SUM over nothing but NULLs is NULL
                L->outs.push_back(WideOut{WideOutKind::Value, acc(agg_op_for(a.fn, at), a.arg, true), -1, want, 1});
            } else if (is_final) {   // avg: (count, sum) states -> sum / count; over no valid value it is NULL
                FG_TRY(need(v, AggFn::Sum, "the AVG count state"));
                const TCol *sm = a.arg2 >= 0 && (size_t)a.arg2 < in.cols.size() ? &in.cols[(size_t)a.arg2] : nullptr;
                if (!sm || sm->c.type != ColType::F64 || (grouped && !sm->present)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: the AVG sum state must be Float64");
                if (!readable(*sm)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: the AVG sum state needs an integer column");
                const int cnt = acc(AggOp::SUM_INT, a.arg, false);
                L->outs.push_back(WideOut{WideOutKind::AvgF64, cnt, acc(AggOp::SUM_F64, a.arg2, false), ColType::F64, 2});
            } else {   // (execute-time messages say AVG, create-time ones avg)
                FG_TRY(need(v, AggFn::Avg, "AVG"));
                const int cnt = acc(AggOp::COUNT, a.arg, true), sum = acc(AggOp::SUM_INT, a.arg, true);
                if (n->single_pass) {   // what Final makes of the one state row: (double) integer sum / (double) count
                    L->outs.push_back(WideOut{WideOutKind::AvgInt, cnt, sum, ColType::F64, 2});
                } else {   // its state: [count UInt64, sum Float64]
                    L->outs.push_back(WideOut{WideOutKind::Value, cnt, -1, ColType::U64, 0});
                    L->outs.push_back(WideOut{WideOutKind::SumAsF64, sum, -1, ColType::F64, 0});
                }
            }
        }
        return FLOCKGPU_OK;
    }

    // ---- no GROUP BY: any list of aggregates, in Partial and Final mode -> ONE row in every case (reduce.hpp): one streaming pass for all
    // accumulators, a fold that writes the row on the device, no wait.  Directly over a filter the filter is not materialised: its predicate pass
    // leaves flag words and the pass reads the filter's input columns under them.
    int exec_global_aggregate(const Node *n, Table *t) {
        Table in;
        const uint32_t *flags = nullptr, *wave_counts = nullptr;
        int32_t flag_tiles = 0;
        std::vector<int> map;
        // (a distinct count reads its argument column as a whole: under it the filter is materialised as ever)
        const Node *f = ir::has_distinct_count(n) ? nullptr : filter_below(n->in[0].get(), &map);
        if (f) {
            Table fin;
            FG_TRY(filter_flags(f, &fin, &flags, &wave_counts, &flag_tiles));
            in.rows = fin.rows;
            in.cols.resize(map.size());
            for (size_t i = 0; i < map.size(); ++i) in.cols[i] = fin.cols[(size_t)map[i]];
        } else {
            FG_TRY(exec(n->in[0].get(), &in));
        }
        if (ir::node_accumulators(n) > kReduceMaxSlots)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: more than %d accumulators in one ungrouped aggregate", kReduceMaxSlots);
        AggLowering L;
        FG_TRY(lower_aggregates(n, in, false, &L));
        // ---- the accumulators as program columns (distinct ones) and slots (distinct ones).  Validity is the column's here, not the accumulator's:
        // a state column that carries validity is read under it.
        ReduceProgram P;
        constexpr uint64_t kSign = 0x8000000000000000ull;
        int pcol[kMaxWideAggs], pslot[kMaxWideAggs];   // per accumulator; -1: no column (nothing but NULLs, or none read) / no slot (a count)
        bool rows_count[kMaxWideAggs];                 // a COUNT that is the count of the selected rows
        bool uns[kMaxWideAggs];
        for (int a = 0; a < L.n_accs; ++a) {
            const AggAcc &A = L.accs[a];
            pcol[a] = pslot[a] = -1;
            uns[a] = false;
            // COUNT(*), and COUNT over a column without validity: the rows selected, no column read.  (The count state of a Partial's AVG over such a
            // column was the column's count, ColCount, before the lowering was shared: the same number -- every selected row reaches the column's
            // slots -- from the same launches.)
            rows_count[a] = A.col < 0 || (A.op == AggOp::COUNT && !in.cols[(size_t)A.col].c.all_null && !in.cols[(size_t)A.col].c.valid);
            if (rows_count[a]) continue;
            const DevColumn &d = in.cols[(size_t)A.col].c;
            uns[a] = d.type == ColType::U64;
            if (d.all_null) continue;
            for (int i = 0; i < P.n_cols; ++i)
                if (P.cols[i].values == d.values && P.cols[i].valid == d.valid && P.cols[i].type == (int32_t)d.type) pcol[a] = i;
            if (pcol[a] < 0) {
                if (P.n_cols == kReduceMaxCols) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: more than %d argument columns in one ungrouped aggregate", kReduceMaxCols);
                P.cols[P.n_cols].values = d.values;
                P.cols[P.n_cols].valid = d.valid;
                P.cols[P.n_cols].type = (int32_t)d.type;
                pcol[a] = P.n_cols++;
            }
            if (A.op == AggOp::COUNT) continue;   // (the pass counts every column's rows)
            ReduceSlot s;
            s.col = pcol[a];
            if (A.op == AggOp::SUM_INT) {
                s.kind = (int32_t)ReduceKind::SumInt;
            } else if (A.op == AggOp::SUM_F64) {
                s.kind = (int32_t)ReduceKind::SumF64;
                s.f64 = 1;
            } else {   // a maximum of order keys; a minimum is the maximum of the complement
                s.kind = (int32_t)ReduceKind::UMax;
                s.inv = A.op == AggOp::MIN_S || A.op == AggOp::MIN_U || A.op == AggOp::MIN_F64;
                s.f64 = A.op == AggOp::MAX_F64 || A.op == AggOp::MIN_F64;
                s.flip = (A.op == AggOp::MAX_U || A.op == AggOp::MIN_U ? 0 : kSign) ^ (s.inv ? ~uint64_t(0) : 0);
            }
            for (int i = 0; i < P.n_slots; ++i)
                if (P.slots[i].kind == s.kind && P.slots[i].col == s.col && P.slots[i].flip == s.flip) pslot[a] = i;
            if (pslot[a] < 0) {
                if (P.n_slots == kReduceMaxSlots) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: more than %d accumulators in one ungrouped aggregate", kReduceMaxSlots);
                P.slots[P.n_slots] = s;
                pslot[a] = P.n_slots++;
            }
        }
        // ---- the result columns as the fold's outputs
        if (L.outs.size() != n->schema.size() || L.outs.size() > (size_t)kReduceMaxOuts)
            return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: an ungrouped aggregate whose schema is not its aggregates'");
        for (const WideOut &w : L.outs) {
            ReduceOut &o = P.outs[P.n_outs++];
            const int a = w.kind == WideOutKind::DistinctCount ? -1 : w.kind == WideOutKind::AvgInt ? w.acc2 : w.acc;   // the accumulator whose column is counted
            o.col = a < 0 ? -1 : pcol[a];
            o.a = a < 0 ? -1 : pslot[a];
            o.b = -1;
            switch (w.kind) {
                case WideOutKind::DistinctCount: o.kind = (int32_t)ReduceOutKind::Rows; break;   // its place in the row, valid: distinct_count_by_group writes the value below
                case WideOutKind::Value:
                    if (L.accs[a].op == AggOp::COUNT) o.kind = (int32_t)(rows_count[a] ? ReduceOutKind::Rows : ReduceOutKind::ColCount);
                    else o.kind = (int32_t)(w.validity ? ReduceOutKind::Value : ReduceOutKind::ValueAlways);
                    break;
                // (back-ends) a UInt64 sum becomes a double as unsigned here; both grouped finishes convert the 64-bit sum as signed
                case WideOutKind::SumAsF64: o.kind = (int32_t)ReduceOutKind::SumAsF64; o.b = uns[a] ? 1 : 0; break;
                case WideOutKind::AvgInt: o.kind = (int32_t)ReduceOutKind::AvgOnePass; o.b = uns[a] ? 1 : 0; break;
                case WideOutKind::AvgF64: o.kind = (int32_t)ReduceOutKind::AvgFinal; o.b = pslot[w.acc2]; break;
            }
        }
        uint64_t *out = nullptr;
        FG_TRY(arena_get_t(ctx, node_key(pl, n, "gagg").c_str(), (size_t)kReduceMaxOuts + kReduceMaxOuts / 8 + 2, &out));
        uint8_t *ov = reinterpret_cast<uint8_t *>(out + kReduceMaxOuts);
        FG_TRY(reduce_global(ctx, node_key(pl, n, "gred").c_str(), P, in.rows, flags, wave_counts, flag_tiles, out, ov));
        // the distinct counts: every row in one group, the count straight into the row (never NULL: the fold marked the place valid)
        for (size_t o = 0; o < L.outs.size(); ++o)
            if (L.outs[o].kind == WideOutKind::DistinctCount)
                FG_TRY(distinct_count_by_group(ctx, node_key(pl, n, "dc", L.outs[o].acc).c_str(), nullptr, 1, in.cols[(size_t)n->aggs[(size_t)L.outs[o].acc].arg].c, in.rows, out + o));
        t->rows = 1;
        t->cols.assign(n->schema.size(), TCol{});
        for (size_t i = 0; i < n->schema.size(); ++i) {
            t->cols[i] = dev_col(n->schema[i].type, out + i, nullptr, 0, n->schema[i].is_ts);
            t->cols[i].c.valid = ov + i;
            t->cols[i].c.nullable = true;
        }
        return FLOCKGPU_OK;
    }

    // ---- no GROUP BY: MAX of one integer column -> one row (NULL over no input)
    int exec_lone_max(const Node *n, const Table &in, Table *t) {
        const ColType at = n->aggs.size() == 1 && n->aggs[0].arg >= 0 ? in.cols[(size_t)n->aggs[0].arg].c.type : ColType::UTF8;
        if (n->aggs.size() != 1 || n->aggs[0].fn != AggFn::Max || at == ColType::UTF8 || at == ColType::F64 || !in.cols[(size_t)n->aggs[0].arg].present)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: global aggregate other than MAX over an integer column");
        const TCol &a = in.cols[(size_t)n->aggs[0].arg];
        int64_t mx = 0;
        int any = 0;
        if (!a.c.all_null) FG_TRY(reduce_max(ctx, a.c, in.rows, &mx, &any));
        int64_t *d = nullptr;
        FG_TRY(arena_get_t(ctx, node_key(pl, n, "max").c_str(), 2, &d));
        // the one value travels as kernel arguments (a host-to-device copy call costs ~10 us of host time; Int32 reads the low word)
        FG_TRY(fill_words(ctx, FillList().add(d, (uint32_t)(uint64_t)mx, 1).add(reinterpret_cast<uint32_t *>(d) + 1, (uint32_t)((uint64_t)mx >> 32), 1)));
        t->rows = 1;
        t->cols[0] = dev_col(at, d, nullptr, 0, a.c.is_ts);
        t->cols[0].c.nullable = true;
        t->cols[0].c.all_null = !any;
        return FLOCKGPU_OK;
    }

    // ---- DISTINCT (Int32, Utf8)
    int exec_distinct_pair(const Node *n, const Table &in, Table *t) {
        const TCol &k = in.cols[(size_t)n->group[0]], &s = in.cols[(size_t)n->group[1]];
        if (k.c.type != ColType::I32 || s.c.type != ColType::UTF8 || !k.present || !s.present)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: two-column GROUP BY other than (Int32, Utf8)");
        if (k.c.valid || s.c.valid) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: DISTINCT over columns that hold NULLs");
        int32_t *rows = nullptr;
        int64_t n_out = 0;
        FG_TRY(distinct_i32_utf8(ctx, node_key(pl, n, "dist").c_str(), static_cast<const int32_t *>(k.c.values),
                                 flockgpu_utf8{s.c.offsets, static_cast<const uint8_t *>(s.c.values)}, in.rows, &rows, &n_out));
        t->rows = n_out;
        FG_TRY(take_column(ctx, node_key(pl, n, "take", 0).c_str(), k.c, rows, n_out, &t->cols[0].c));
        FG_TRY(take_column(ctx, node_key(pl, n, "take", 1).c_str(), s.c, rows, n_out, &t->cols[1].c));
        t->cols[0].present = t->cols[1].present = true;
        return FLOCKGPU_OK;
    }

    // ---- the key shapes of GROUP BY, chosen once per execute from the node and its input's columns
    enum class KeyShape {
        Int,              // one Int32 / Int64 / UInt64 / Timestamp column: the dense (direct-address) table where number_groups finds it fits, else the hashed one
        Utf8,             // one Utf8 column, grouped on its dictionary codes: dense by construction where the accumulators allow, else hashed
        PairI32,          // (Int32, Int32) without NULLs, packed into one 64-bit key
        DistinctI32Utf8,  // DISTINCT (Int32, Utf8): no aggregates
        Composite,        // ids of composite keys (relops.hpp key_codes), groups in order of first appearance: three or more columns, two other than the
                          // pairs above, NULLs in a two-column key -- and every node that needs the ids themselves (a distinct count; more than
                          // kMaxGroupAggs accumulators), whatever its key
    };
    struct KeyPlan {
        KeyShape shape = KeyShape::Composite;
        // NULL group keys form ONE group (DataFusion groups NULLs together): an Int32 key column widened to 64 bits has room for a value no Int32
        // takes (kNullKey), and so have a Utf8 column's dictionary codes (row numbers) ...
        bool null_keys = false;
        // ... and a 64-bit key (Int64 / UInt64 / Timestamp) hands its validity to the GROUP BY itself, which keeps the NULLs in a slot of their own
        bool null_in_table = false;
    };
    static constexpr int64_t kNullKey = int64_t(1) << 40;
    int choose_key_shape(const Node *n, const Table &in, bool needs_ids, KeyPlan *kp) {
        bool composite = n->group.size() > 2 || needs_ids;
        if (n->group.size() == 2 && !needs_ids) {
            const TCol &a = in.cols[(size_t)n->group[0]], &b = in.cols[(size_t)n->group[1]];
            composite = a.c.type != ColType::I32 || a.c.valid || b.c.valid || b.c.type != (n->aggs.empty() ? ColType::UTF8 : ColType::I32);
            if (a.c.type == ColType::F64 || b.c.type == ColType::F64) composite = false;   // (refused by the pair's own path, with its message)
        }
        if (composite) {
            if (n->group.size() > (size_t)kMaxKeyCols) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: GROUP BY more than %d columns", kMaxKeyCols);
            for (int c : n->group)
                if (in.cols[(size_t)c].c.type == ColType::F64) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: GROUP BY a Float64 column");
            kp->shape = KeyShape::Composite;
            return FLOCKGPU_OK;
        }
        const TCol &k = in.cols[(size_t)n->group[0]];
        if (n->group.size() == 2) kp->shape = n->aggs.empty() ? KeyShape::DistinctI32Utf8 : KeyShape::PairI32;
        else kp->shape = k.c.type == ColType::UTF8 ? KeyShape::Utf8 : KeyShape::Int;
        if (kp->shape == KeyShape::DistinctI32Utf8) return FLOCKGPU_OK;
        kp->null_keys = k.c.valid != nullptr;
        if (kp->null_keys && kp->shape == KeyShape::PairI32) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: NULLs in a two-column GROUP BY key");
        kp->null_in_table = kp->null_keys && kp->shape == KeyShape::Int && k.c.type != ColType::I32;
        return FLOCKGPU_OK;
    }

    // ---- number the groups: runs the table the key shape takes over `specs`.  *gid: the rows' group ids (Composite alone).
    int number_groups(const Node *n, const Table &in, const KeyPlan &kp, const AggSpec *specs, int n_specs, GroupResultN *g, const int32_t **gid) {
        if (kp.shape == KeyShape::Composite) return group_composite(n, in, specs, n_specs, g, gid);
        const TCol &k = in.cols[(size_t)n->group[0]];
        // A dense key without NULLs under integer accumulators without NULLs: the perfect-hash GROUP BY (relops.hpp "dense integer keys").
        // Everything else (two-column keys, NULLs, Float64 accumulators, keys spread wider than their row count) takes the hash table.
        const bool fit = specs_fit_dense(specs, n_specs) && !kp.null_keys && k.present && in.rows > 0;
        int64_t *keys = nullptr;   // the hash table's: every key normalised to one int64 per row
        if (kp.shape == KeyShape::PairI32) {
            const TCol &k2 = in.cols[(size_t)n->group[1]];
            if (k.c.type != ColType::I32 || k2.c.type != ColType::I32 || !k.present || !k2.present)
                return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: two-column GROUP BY other than (Int32, Int32) / (Int32, Utf8)");
            if (k2.c.valid) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: NULLs in a two-column GROUP BY key");
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "gk").c_str(), (size_t)in.rows + 2, &keys));
            FG_TRY(pack_i32_pair(ctx, static_cast<const int32_t *>(k.c.values), static_cast<const int32_t *>(k2.c.values), in.rows, keys));
        } else if (kp.shape == KeyShape::Utf8) {   // group on the strings' dictionary codes; the key column is taken from the first rows
            if (!k.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: key column was not materialised");
            FG_TRY(arena_get_t(ctx, node_key(pl, n, "gk").c_str(), (size_t)in.rows + 2, &keys));
            FG_TRY(utf8_codes(ctx, node_key(pl, n, "codes").c_str(), k.c, in.rows, keys, nullptr, 0, nullptr));
            // The codes are row numbers of the key's own relation: dense by construction.  The code of a group IS a row that carries the group's
            // string, so it also stands in for the first row the key column is taken from.
            if (fit && in.rows < (int64_t(1) << 31)) {
                FG_TRY(group_by_dense(ctx, node_key(pl, n, "grp").c_str(), plain_col(ColType::I64, keys), in.rows, 0, in.rows - 1, specs, n_specs, g));
                int32_t *rep = nullptr;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "rep").c_str(), (size_t)g->n_groups + 4, &rep));
                FG_TRY(narrow_i64_to_i32(ctx, g->keys, g->n_groups, rep));
                g->first_row = rep;
                return FLOCKGPU_OK;
            }
            // (a NULL's bytes are whatever its slot holds -- usually nothing, which is also the empty string's code: NULLs get their own key;
            // the group's key comes out NULL through the validity of its first row, write_key_columns)
            if (kp.null_keys) FG_TRY(replace_invalid_i64(ctx, keys, k.c.valid, in.rows, kNullKey));
        } else {
            // slot = key - min over the column's exact range: no hashing, no int64 copy of the key column
            if (fit && (k.c.type == ColType::I32 || k.c.type == ColType::I64 || k.c.type == ColType::U64) && stats_worth_it(k, in.rows)) {
                int64_t kmin = 0, kmax = 0;
                FG_TRY(int_col_stats(k, in.rows, &kmin, &kmax));
                if (dense_range_ok(kmin, kmax, in.rows, k.c.type == ColType::U64)) return group_by_dense(ctx, node_key(pl, n, "grp").c_str(), k.c, in.rows, kmin, kmax, specs, n_specs, g);
            }
            if (k.c.type == ColType::F64) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: GROUP BY a Float64 column");
            FG_TRY(key_i64(n, k, in.rows, "gk", &keys));
            if (kp.null_keys && !kp.null_in_table) FG_TRY(replace_invalid_i64(ctx, keys, k.c.valid, in.rows, kNullKey));
        }
        return group_by_key64_n(ctx, node_key(pl, n, "grp").c_str(), keys, in.rows, specs, n_specs, g, kp.null_in_table ? k.c.valid : nullptr);
    }

    // ---- the key columns of the groups
    int write_key_columns(const Node *n, const Table &in, const KeyPlan &kp, const GroupResultN &g, Table *t) {
        const TCol &k = in.cols[(size_t)n->group[0]];
        switch (kp.shape) {
            case KeyShape::Composite:   // each group's key values are those of its first row (validity taken along)
                for (size_t c = 0; c < n->group.size(); ++c) {
                    const TCol &src = in.cols[(size_t)n->group[c]];
                    FG_TRY(take_column(ctx, node_key(pl, n, "take", (int)c).c_str(), src.c, g.first_row, g.n_groups, &t->cols[c].c));
                    t->cols[c].present = true;
                    t->cols[c].c.is_ts = n->schema[c].is_ts;
                    t->cols[c].c.nullable = n->schema[c].nullable;
                }
                break;
            case KeyShape::PairI32: {
                int32_t *ka = nullptr, *kb = nullptr;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "nk").c_str(), (size_t)g.n_groups + 4, &ka));
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "nk2").c_str(), (size_t)g.n_groups + 4, &kb));
                FG_TRY(unpack_i32_pair(ctx, g.keys, g.n_groups, ka, kb));
                t->cols[0] = dev_col(ColType::I32, ka);
                t->cols[1] = dev_col(ColType::I32, kb);
                t->cols[1].c.nullable = n->schema[1].nullable;
                break;
            }
            case KeyShape::Utf8:
                FG_TRY(take_column(ctx, node_key(pl, n, "take", 0).c_str(), k.c, g.first_row, g.n_groups, &t->cols[0].c));
                t->cols[0].present = true;
                break;
            case KeyShape::DistinctI32Utf8: break;   // (exec_distinct_pair writes its own)
            case KeyShape::Int:
                if (k.c.type == ColType::I32) {
                    int32_t *nk = nullptr;
                    FG_TRY(arena_get_t(ctx, node_key(pl, n, "nk").c_str(), (size_t)g.n_groups + 4, &nk));
                    FG_TRY(narrow_i64_to_i32(ctx, g.keys, g.n_groups, nk));
                    t->cols[0] = dev_col(ColType::I32, nk);
                    if (kp.null_keys) {   // the NULL group's key is NULL again
                        uint8_t *kv = nullptr;
                        FG_TRY(arena_get_t(ctx, node_key(pl, n, "nkv").c_str(), (size_t)g.n_groups + 16, &kv));
                        FG_TRY(valid_from_i64(ctx, g.keys, g.n_groups, kNullKey, kv));
                        t->cols[0].c.valid = kv;
                    }
                } else {
                    t->cols[0] = dev_col(k.c.type, g.keys, nullptr, 0, k.c.is_ts);
                    if (kp.null_in_table) t->cols[0].c.valid = g.key_valid;
                }
                if (!kp.null_keys) t->cols[0].subset_of = k.subset_of ? k.subset_of : k.c.values;   // (a group's key is one of the input's keys)
                break;
        }
        t->cols[0].c.nullable = n->schema[0].nullable;
        return FLOCKGPU_OK;
    }

    // ---- the result columns of the groups, from the accumulators of one of the tables (g.agg) -- or, `wide`, of the one pass over the ids, which
    // runs here and finishes every column but the distinct counts on the device.  The distinct counts run over the ids in both cases.
    int write_result_columns(const Node *n, const Table &in, const AggLowering &L, const AggSpec *specs, const GroupResultN &g, const int32_t *gid, bool wide, Table *t) {
        const int64_t G = g.n_groups;
        WideGroupResult wres;
        std::vector<int> wide_col(L.outs.size(), -1);   // per result column: its place among the wide pass's (it takes no distinct count)
        if (wide) {
            WideOut wo[kMaxWideAggs];
            int n_wo = 0;
            for (size_t o = 0; o < L.outs.size(); ++o)
                if (L.outs[o].kind != WideOutKind::DistinctCount) wo[wide_col[o] = n_wo++] = L.outs[o];
            FG_TRY(group_by_ids_wide(ctx, node_key(pl, n, "wide").c_str(), gid, in.rows, G, specs, L.n_accs, wo, n_wo, &wres));
        }
        for (size_t o = 0; o < L.outs.size(); ++o) {
            const WideOut &w = L.outs[o];
            const size_t oc = n->group.size() + o;
            const int col = (int)oc;
            TCol &out = t->cols[oc];
            if (w.kind == WideOutKind::DistinctCount) {
                uint64_t *dc = nullptr;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "av", col).c_str(), (size_t)G + 2, &dc));
                if (G > 0) FG_TRY(distinct_count_by_group(ctx, node_key(pl, n, "dc", w.acc).c_str(), gid, G, in.cols[(size_t)n->aggs[(size_t)w.acc].arg].c, in.rows, dc));
                out = dev_col(ColType::U64, dc);
            } else if (wide) {
                out = dev_col(n->schema[oc].type, wres.col[wide_col[o]], nullptr, 0, n->schema[oc].is_ts);
                out.c.valid = wres.valid[wide_col[o]];
            } else if (w.kind == WideOutKind::Value) {
                if (w.type == ColType::I32) {
                    int32_t *v = nullptr;
                    FG_TRY(arena_get_t(ctx, node_key(pl, n, "av", col).c_str(), (size_t)G + 4, &v));
                    FG_TRY(narrow_i64_to_i32(ctx, reinterpret_cast<const int64_t *>(g.agg[w.acc]), G, v));
                    out = dev_col(ColType::I32, v);
                } else {
                    out = dev_col(w.type, g.agg[w.acc], nullptr, 0, n->schema[oc].is_ts);
                }
                if (w.validity == 1) out.c.valid = g.agg_valid[w.acc];   // (null where the argument carried no validity)
            } else if (w.kind == WideOutKind::SumAsF64) {   // the sum state of a Partial's AVG
                // (back-ends) the 64-bit integer sum becomes a double as signed, here and in the wide finish; the ungrouped fold converts a UInt64 sum as unsigned
                double *sum = nullptr;
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "av", col).c_str(), (size_t)G + 2, &sum));
                FG_TRY(i64_to_f64(ctx, reinterpret_cast<const int64_t *>(g.agg[w.acc]), G, sum));
                out = dev_col(ColType::F64, sum);
            } else {   // AVG finished: sum / count, NULL over no valid value
                const double *sum = reinterpret_cast<const double *>(g.agg[w.acc2]);   // (AvgF64: the Float64 sum of the states)
                double *avg = nullptr;
                uint8_t *av = nullptr;
                if (w.kind == WideOutKind::AvgInt) {   // (signed, as above)
                    double *s = nullptr;
                    FG_TRY(arena_get_t(ctx, node_key(pl, n, "avs", col).c_str(), (size_t)G + 2, &s));
                    FG_TRY(i64_to_f64(ctx, reinterpret_cast<const int64_t *>(g.agg[w.acc2]), G, s));
                    sum = s;
                }
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "av", col).c_str(), (size_t)G + 2, &avg));
                FG_TRY(arena_get_t(ctx, node_key(pl, n, "avv", col).c_str(), (size_t)G + 16, &av));
                FG_TRY(avg_finish(ctx, sum, g.agg[w.acc], G, avg));
                FG_TRY(valid_from_i64(ctx, reinterpret_cast<const int64_t *>(g.agg[w.acc]), G, 0, av));
                out = dev_col(ColType::F64, avg);
                out.c.valid = av;
            }
            out.c.nullable = true;
        }
        return FLOCKGPU_OK;
    }

    int exec_aggregate(const Node *n, Table *t) {
        const Node *partial = nullptr;
        if (final_is_identity(n, &partial)) {
            FG_TRY(exec(partial, t));
            for (size_t i = 0; i < n->schema.size() && i < t->cols.size(); ++i) {
                t->cols[i].c.is_ts = n->schema[i].is_ts;
                t->cols[i].c.nullable = n->schema[i].nullable;
            }
            return FLOCKGPU_OK;
        }
        if (n->group.empty() && !ir::lone_integer_max(n)) return exec_global_aggregate(n, t);
        Table in;
        FG_TRY(exec(n->in[0].get(), &in));
        t->cols.assign(n->schema.size(), TCol{});
        for (size_t i = 0; i < n->schema.size(); ++i) {
            t->cols[i].c.type = n->schema[i].type;
            t->cols[i].c.is_ts = n->schema[i].is_ts;
            t->cols[i].c.nullable = n->schema[i].nullable;
        }
        if (n->group.empty()) return exec_lone_max(n, in, t);
        // five or more accumulators go through one pass over group ids (groupwide.hpp), and a distinct count runs over ids too
        const bool wide = ir::node_accumulators(n) > kMaxGroupAggs;
        KeyPlan kp;
        FG_TRY(choose_key_shape(n, in, wide || ir::has_distinct_count(n), &kp));
        if (kp.shape == KeyShape::DistinctI32Utf8) return exec_distinct_pair(n, in, t);
        // Partial: accumulators over the rows -> state columns (agg_state_cols); Final: the same accumulators over the states
        AggLowering L;
        FG_TRY(lower_aggregates(n, in, true, &L));
        AggSpec specs[kMaxWideAggs];   // a COUNT reads validity alone
        for (int a = 0; a < L.n_accs; ++a) {
            const AggAcc &A = L.accs[a];
            const DevColumn *d = A.col >= 0 ? &in.cols[(size_t)A.col].c : nullptr;
            specs[a] = A.op == AggOp::COUNT ? AggSpec{A.op, nullptr, ColType::I64, d ? d->valid : nullptr} : AggSpec{A.op, d->values, d->type, A.with_valid ? d->valid : nullptr};
        }
        GroupResultN g;
        const int32_t *gid = nullptr;
        FG_TRY(number_groups(n, in, kp, specs, wide ? 0 : L.n_accs, &g, &gid));   // (wide: the ids and first rows only)
        t->rows = g.n_groups;
        FG_TRY(write_key_columns(n, in, kp, g, t));
        return write_result_columns(n, in, L, specs, g, gid, wide, t);
    }
};

// ------------------------------------------------------------------ Arrow export
struct BatchPriv {
    std::shared_ptr<HostBlock> block;
    std::vector<const void *> buffers;
    std::vector<ArrowArray *> child_ptrs;
    std::vector<std::unique_ptr<ArrowArray>> children;
    std::vector<std::unique_ptr<BatchPriv>> child_priv;
};
void release_child(ArrowArray *a) {
    if (a) a->release = nullptr;  // memory belongs to the parent struct array
}
void release_batch(ArrowArray *a) {
    if (!a || !a->release) return;
    BatchPriv *p = static_cast<BatchPriv *>(a->private_data);
    if (p) {
        for (auto &c : p->children)
            if (c && c->release) c->release(c.get());
        delete p;
    }
    a->release = nullptr;
}
// Arrow C Data Interface metadata: int32 pair count, then per pair int32 key length, key, int32 value length, value (native endian)
std::string encode_metadata(const char *key, const char *value) {
    std::string m;
    auto put = [&](int32_t v) { m.append(reinterpret_cast<const char *>(&v), 4); };
    put(1);
    put((int32_t)strlen(key));
    m += key;
    put((int32_t)strlen(value));
    m += value;
    return m;
}

struct SchemaPriv {
    std::string format, name, metadata;
    std::vector<ArrowSchema *> child_ptrs;
    std::vector<std::unique_ptr<ArrowSchema>> children;
};
void release_schema(ArrowSchema *s) {
    if (!s || !s->release) return;
    SchemaPriv *p = static_cast<SchemaPriv *>(s->private_data);
    if (p) {
        for (auto &c : p->children)
            if (c && c->release) c->release(c.get());
        delete p;
    }
    s->release = nullptr;
}
void make_schema(ArrowSchema *s, const char *format, const char *name, bool nullable) {
    SchemaPriv *p = new SchemaPriv();
    p->format = format;
    p->name = name;
    std::memset(s, 0, sizeof *s);
    s->format = p->format.c_str();
    s->name = p->name.c_str();
    s->flags = nullable ? ARROW_FLAG_NULLABLE : 0;
    s->release = release_schema;
    s->private_data = p;
}
void add_schema_child(ArrowSchema *parent, const char *format, const char *name, bool nullable) {
    SchemaPriv *p = static_cast<SchemaPriv *>(parent->private_data);
    p->children.emplace_back(new ArrowSchema());
    make_schema(p->children.back().get(), format, name, nullable);
    p->child_ptrs.push_back(p->children.back().get());
    parent->children = p->child_ptrs.data();
    parent->n_children = (int64_t)p->child_ptrs.size();
}
void export_schema(const Node *root, ArrowSchema *out, bool shuffled = false) {
    make_schema(out, "+s", "", false);
    if (shuffled) {   // the partitions of a shuffling stage say how their rows were placed (flockgpu_plan.h "hash placement")
        SchemaPriv *p = static_cast<SchemaPriv *>(out->private_data);
        p->metadata = encode_metadata(kPartitionSchemeKey, kPartitionScheme);
        out->metadata = p->metadata.data();
    }
    for (auto &f : root->schema) {
        DevColumn c;
        c.type = f.type;
        c.is_ts = f.is_ts;
        add_schema_child(out, format_of(c), f.name.c_str(), f.nullable);
    }
}

// Copies the table's buffers into ONE pinned block (async, then a single synchronisation) and exposes `n_parts`
// record batches over it: batch p = rows [part_off[p], part_off[p + 1]) through the Arrow `offset` field of its children.
int export_batches(flockgpu_ctx *ctx, const Table &t, const std::vector<int64_t> &part_off, ArrowArray *out_batches) {
    const int n_parts = (int)part_off.size() - 1;
    struct Slot { size_t at = 0, bytes = 0; const void *dev = nullptr; };
    std::vector<Slot> values(t.cols.size()), offsets(t.cols.size()), validity(t.cols.size()), valid_bytes(t.cols.size());
    size_t total = 0;
    auto reserve = [&](Slot &s, const void *dev, size_t bytes) {
        s.at = total;
        s.bytes = bytes;
        s.dev = dev;
        total += (bytes + 63) & ~size_t(63);
    };
    for (size_t i = 0; i < t.cols.size(); ++i) {
        const TCol &c = t.cols[i];
        if (!c.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: output column %zu was not materialised", i);
        if (c.c.type == ColType::UTF8) {
            reserve(offsets[i], c.c.offsets, (size_t)(t.rows + 1) * 4);
            reserve(values[i], c.c.values, (size_t)std::max<int64_t>(c.c.bytes, 0));
        } else {
            reserve(values[i], c.c.values, (size_t)t.rows * col_width(c.c.type));
        }
        if (c.c.all_null || c.c.valid) reserve(validity[i], nullptr, (size_t)(t.rows + 7) / 8 + 8);
        if (c.c.valid && !c.c.all_null) reserve(valid_bytes[i], c.c.valid, (size_t)t.rows);   // one byte per row on the device: packed into bits below
    }
    auto block = std::make_shared<HostBlock>();
    block->ptr = pool().get(std::max<size_t>(total, 64), &block->cap);
    if (!block->ptr) return fail(ctx, FLOCKGPU_ERR_OOM, "plan execute: pinned host allocation of %zu bytes failed", total);
    uint8_t *base = static_cast<uint8_t *>(block->ptr);
    for (auto *group : {&values, &offsets, &valid_bytes})
        for (auto &s : *group)
            if (s.bytes && s.dev) FG_HIP(ctx, hipMemcpyAsync(base + s.at, s.dev, s.bytes, hipMemcpyDeviceToHost, ctx->stream));
    for (auto &s : validity)
        if (s.bytes) std::memset(base + s.at, 0, s.bytes);
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < t.cols.size(); ++i)   // validity bytes -> the Arrow bitmap (bit r of the column = row r; batches address it through `offset`)
        if (valid_bytes[i].bytes) {
            const uint8_t *vb = base + valid_bytes[i].at;
            uint8_t *bits = base + validity[i].at;
            for (int64_t r = 0; r < t.rows; ++r)
                if (vb[r]) bits[r >> 3] |= (uint8_t)(1u << (r & 7));
        }
    for (int p = 0; p < n_parts; ++p) {
        ArrowArray *a = &out_batches[p];
        BatchPriv *bp = new BatchPriv();
        bp->block = block;
        std::memset(a, 0, sizeof *a);
        const int64_t lo = part_off[(size_t)p], len = part_off[(size_t)p + 1] - lo;
        a->length = len;
        bp->buffers = {nullptr};
        a->n_buffers = 1;
        a->buffers = bp->buffers.data();
        for (size_t i = 0; i < t.cols.size(); ++i) {
            const TCol &c = t.cols[i];
            bp->children.emplace_back(new ArrowArray());
            bp->child_priv.emplace_back(new BatchPriv());
            ArrowArray *ch = bp->children.back().get();
            BatchPriv *cp = bp->child_priv.back().get();
            std::memset(ch, 0, sizeof *ch);
            ch->length = len;
            ch->offset = lo;
            const bool has_bitmap = c.c.all_null || (c.c.valid && t.rows > 0);
            const void *valid = has_bitmap ? base + validity[i].at : nullptr;
            ch->null_count = c.c.all_null ? len : 0;
            if (!c.c.all_null && valid_bytes[i].bytes) {
                const uint8_t *vb = base + valid_bytes[i].at;
                int64_t nulls = 0;
                for (int64_t r = lo; r < lo + len; ++r) nulls += vb[r] ? 0 : 1;
                ch->null_count = nulls;
            }
            if (c.c.type == ColType::UTF8) cp->buffers = {valid, base + offsets[i].at, base + values[i].at};
            else cp->buffers = {valid, base + values[i].at};
            ch->n_buffers = (int64_t)cp->buffers.size();
            ch->buffers = cp->buffers.data();
            ch->release = release_child;
            bp->child_ptrs.push_back(ch);
        }
        a->children = bp->child_ptrs.data();
        a->n_children = (int64_t)bp->child_ptrs.size();
        a->release = release_batch;
        a->private_data = bp;
    }
    return FLOCKGPU_OK;
}

int run_plan(flockgpu_plan *plan, bool partitioned, ArrowSchema *out_schema, ArrowArray *out_batches, int capacity, int *n_out) {
    flockgpu_ctx *ctx = plan->ctx;
    FG_HIP(ctx, hipSetDevice(ctx->device));
    const Node *root = plan->ir.root.get();
    Exec ex{plan, ctx};
    Table t;
    std::vector<int64_t> part_off;
    if (partitioned && root->kind == NKind::Repartition) {
        if (root->n_parts > capacity) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: %d output partitions, room for %d", root->n_parts, capacity);
        // Filter -> Repartition (stage 0 of planner.rs:152-171: the rows a filter keeps are what travels): the filter's row selection
        // and the partition's send order are COMPOSED and the columns taken once, from the filter's input -- materialising the
        // filtered table first moved every column twice (the three Utf8 columns of q3's persons among them)
        const Node *below = root->in[0].get();
        while (below->kind == NKind::Repartition) below = below->in[0].get();
        const bool compose = below->kind == NKind::Filter && plan->fused[(size_t)below->id].kind == kNone && below->schema.size() == root->schema.size() &&
                             root->in[0]->schema.size() == root->schema.size();
        Table in;
        int32_t *sel = nullptr;      // compose: rows of `in` the filter keeps
        int64_t n_sel = 0;
        if (compose) FG_TRY(ex.filter_rows(below, &in, &sel, &n_sel));
        else FG_TRY(ex.exec(root->in[0].get(), &in));
        const int64_t n_rows = compose ? n_sel : in.rows;
        // RepartitionExec Hash(exprs, n): equal keys must meet in one partition; hashing the first key column already
        // guarantees that, and which partition a key lands on is unobservable
        TCol k = in.cols[(size_t)root->hash_cols[0]];
        if (!k.present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: key column was not materialised");
        if (compose) FG_TRY(take_column(ctx, node_key(plan, root, "pkcol").c_str(), in.cols[(size_t)root->hash_cols[0]].c, sel, n_sel, &k.c));
        int64_t *keys = nullptr;
        if (k.c.type == ColType::UTF8) {
            FG_TRY(arena_get_t(ctx, node_key(plan, root, "pk").c_str(), (size_t)n_rows + 2, &keys));
            FG_TRY(hash_utf8_i64(ctx, k.c, n_rows, keys));
        } else {
            FG_TRY(ex.key_i64(root, k, n_rows, "pk", &keys));
        }
        if (k.c.valid) FG_TRY(replace_invalid_i64(ctx, keys, k.c.valid, n_rows, 0));   // (NULL keys: one key as far as placement goes; the slot's bytes are unspecified)
        int32_t *rows = nullptr;
        if (root->hash_diff) {
            // HashDiff(exprs, n): every DISTINCT key a partition of its own (session.rs:236-253: n is COUNT(DISTINCT key), counted by the host
            // just before).  A stable sort of the rows by the key groups them, input order kept inside a key; the partitions come out in key
            // order (which partition a key gets is as unobservable as under Hash).  More distinct keys than n: the host's count does not fit
            // the data -- refused; fewer: the partitions behind the last key are empty.
            if (k.c.type == ColType::UTF8 || k.c.type == ColType::F64) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: HashDiff on a key that is not an integer column");
            if (k.c.valid) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: HashDiff on a key column that holds NULLs");
            if (root->hash_cols.size() != 1) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan execute: HashDiff on more than one key column");
            const SortKey sk{k.c, false, false};
            FG_TRY(sort_rows(ctx, node_key(plan, root, "hdsort").c_str(), &sk, 1, n_rows, &rows));
            int32_t *starts = nullptr;
            int64_t n_keys = 0;
            FG_TRY(key_run_starts(ctx, node_key(plan, root, "hdruns").c_str(), keys, rows, n_rows, &starts, &n_keys));
            if (n_keys > root->n_parts)
                return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: HashDiff names %d partitions, the key column holds %lld distinct keys", root->n_parts, (long long)n_keys);
            std::vector<int32_t> h_starts((size_t)n_keys);
            if (n_keys) {
                FG_HIP(ctx, hipMemcpyAsync(h_starts.data(), starts, sizeof(int32_t) * (size_t)n_keys, hipMemcpyDeviceToHost, ctx->stream));
                FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
            part_off.assign((size_t)root->n_parts + 1, n_rows);
            for (int64_t g = 0; g < n_keys; ++g) part_off[(size_t)g] = h_starts[(size_t)g];
        } else
        FG_TRY(partition_rows_key64(ctx, node_key(plan, root, "part").c_str(), keys, n_rows, root->n_parts, &rows, &part_off));
        if (compose) {   // send order over the filter's input: sel[rows[i]]
            int32_t *composed = nullptr;
            FG_TRY(arena_get_t(ctx, node_key(plan, root, "rows").c_str(), (size_t)n_rows + 4, &composed));
            FG_TRY(gather_i32(ctx, sel, rows, n_rows, composed));
            rows = composed;
        }
        t.rows = n_rows;
        t.cols.assign(root->schema.size(), TCol{});
        FG_TRY(ex.take_table(root, in, std::vector<char>(root->schema.size(), 1), rows, n_rows, 0, &t));
    } else {
        FG_TRY(ex.exec(root, &t));
        part_off = {0, t.rows};
    }
    if ((int)part_off.size() - 1 > capacity) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: no room for the output batch");
    FG_TRY(export_batches(ctx, t, part_off, out_batches));
    plan->fed_bytes = 0;  // export synchronised the stream: every borrowed buffer has been read
    export_schema(root, out_schema, partitioned && root->kind == NKind::Repartition);
    *n_out = (int)part_off.size() - 1;
    return FLOCKGPU_OK;
}

}  // namespace

extern "C" {

int flockgpu_plan_create_ex(flockgpu_ctx *ctx, const char *plan_json, size_t len, uint32_t flags, flockgpu_plan **out) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!plan_json || !out) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_create: null argument");
    if (flags & ~FLOCKGPU_PLAN_GENERIC_ONLY) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_create: unknown flag bits 0x%x", flags & ~FLOCKGPU_PLAN_GENERIC_ONLY);
    *out = nullptr;
    std::unique_ptr<flockgpu_plan> pl(new flockgpu_plan());
    pl->ctx = ctx;
    FG_TRY(parse_and_build(ctx, plan_json, len, pl.get(), flags));
    *out = pl.release();
    return FLOCKGPU_OK;
}

int flockgpu_plan_create(flockgpu_ctx *ctx, const char *plan_json, size_t len, flockgpu_plan **out) {
    return flockgpu_plan_create_ex(ctx, plan_json, len, 0, out);
}

int flockgpu_plan_recognise(const char *plan_json, size_t len, int *query) {
    if (!plan_json || !query) return FLOCKGPU_ERR_INVALID;
    flockgpu_plan pl;
    const int rc = parse_and_build(nullptr, plan_json, len, &pl);
    if (rc != FLOCKGPU_OK) return rc;
    *query = pl.query;
    return FLOCKGPU_OK;
}

int flockgpu_plan_explain(const char *plan_json, size_t len, char *out, size_t capacity) {
    if (!plan_json || !out || !capacity) return FLOCKGPU_ERR_INVALID;
    flockgpu_plan pl;
    const int rc = parse_and_build(nullptr, plan_json, len, &pl);
    const std::string text = rc == FLOCKGPU_OK ? pl.description : (rc == FLOCKGPU_ERR_UNSUPPORTED ? "unsupported: " + pl.ir.why : std::string("plan JSON error"));
    snprintf(out, capacity, "%s", text.c_str());
    return rc;
}

void flockgpu_plan_destroy(flockgpu_plan *plan) {
    if (!plan) return;
#ifdef FLOCKGPU_EXPERIMENTAL
    if (plan->ring_ppw) ApiClock::dump();
#endif
    flockgpu_ctx *ctx = plan->ctx;
    prefetch_drop(plan);
    if (plan->copy_stream) {
        (void)hipStreamSynchronize(plan->copy_stream);
        (void)hipStreamDestroy(plan->copy_stream);
        (void)hipEventDestroy(plan->copy_done);
        (void)hipEventDestroy(plan->append_done);
    }
    if (plan->async_pending) {   // an execute nobody waited for: let it finish, drop what it produced
        if (ctx_wait(ctx) == FLOCKGPU_OK) {
            for (int i = 0; i < plan->async_n; ++i)
                if (plan->async_batches[(size_t)i].release) plan->async_batches[(size_t)i].release(&plan->async_batches[(size_t)i]);
            if (plan->async_schema.release) plan->async_schema.release(&plan->async_schema);
        }
        plan->async_pending = false;
        if (ctx->plan_in_flight == plan) ctx->plan_in_flight = nullptr;
    }
    (void)hipStreamSynchronize(ctx->stream);
    char prefix[64];
    snprintf(prefix, sizeof prefix, "plan%p.", (const void *)plan);
    for (auto it = ctx->arena.begin(); it != ctx->arena.end();) {
        if (it->first.compare(0, strlen(prefix), prefix) == 0) {
            if (it->second.ptr) dev_free(ctx, it->second.ptr);
            it = ctx->arena.erase(it);
        } else {
            ++it;
        }
    }
    // host-side caches keyed by the same names (tile schedules of scan.hpp) describe buffers that no longer exist
    for (auto it = ctx->host_i64.begin(); it != ctx->host_i64.end();) it = it->first.compare(0, strlen(prefix), prefix) == 0 ? ctx->host_i64.erase(it) : std::next(it);
    for (auto it = ctx->host_u64.begin(); it != ctx->host_u64.end();) it = it->first.compare(0, strlen(prefix), prefix) == 0 ? ctx->host_u64.erase(it) : std::next(it);
    for (auto it = ctx->pinned.begin(); it != ctx->pinned.end();) {
        if (it->first.compare(0, strlen(prefix), prefix) == 0) {
            if (it->second.ptr) (void)hipHostFree(it->second.ptr);
            it = ctx->pinned.erase(it);
        } else {
            ++it;
        }
    }
    for (int k = 0; k < kStageChunks; ++k) {
        if (plan->stage[k]) (void)hipHostFree(plan->stage[k]);
        if (plan->stage_done[k]) (void)hipEventDestroy(plan->stage_done[k]);
    }
    delete plan;
}

int flockgpu_plan_query(const flockgpu_plan *plan) { return plan ? plan->query : 0; }
const char *flockgpu_plan_description(const flockgpu_plan *plan) { return plan ? plan->description.c_str() : nullptr; }
int flockgpu_plan_num_inputs(const flockgpu_plan *plan) { return plan ? (int)plan->ir.leaves.size() : 0; }
const char *flockgpu_plan_input_name(const flockgpu_plan *plan, int input) {
    if (!plan || input < 0 || input >= (int)plan->ir.leaves.size()) return nullptr;
    return plan->ir.leaves[(size_t)input].relation.c_str();
}
int flockgpu_plan_output_partitions(const flockgpu_plan *plan) {
    if (!plan) return 0;
    return plan->ir.root->kind == NKind::Repartition ? plan->ir.root->n_parts : 1;
}
int flockgpu_plan_is_shuffling(const flockgpu_plan *plan) { return plan && plan->ir.root->kind == NKind::Repartition ? 1 : 0; }

// The tail of execute_retain, shared with flockgpu_plan_exchange_retain's one-rank case: `t` becomes the plan's retained result.
static int keep_result(flockgpu_plan *plan, Table &t, int64_t *rows) {
    flockgpu_ctx *ctx = plan->ctx;
    const Node *root = plan->ir.root.get();
    if (t.cols.size() != root->schema.size()) return fail(ctx, FLOCKGPU_ERR_HIP, "plan execute: %zu result columns for a schema of %zu", t.cols.size(), root->schema.size());
    for (size_t c = 0; c < t.cols.size(); ++c)
        if (!t.cols[c].present) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: output column '%s' was not materialised", root->schema[c].name.c_str());
    // A result column must outlive the executes of OTHER plans on this context.  Buffers named after this plan (its leaves, its
    // generic operators' outputs) do; a fused pipeline that hands out context-wide buffers ("q5.out_auction", ...) would have them
    // overwritten by the same pipeline inside another plan -- q5's two stage plans both run the fused Partial COUNT (today its
    // columns reach the plan's result through plan-named buffers; this keeps it that way for whatever is fused next).  Such a column
    // is copied into a buffer of this plan (device to device, stream-ordered).
    char prefix[40];
    snprintf(prefix, sizeof prefix, "plan%p.", (const void *)plan);
    auto mine = [&](const void *ptr) {
        if (!ptr) return true;
        const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
        for (auto it = ctx->arena.lower_bound(prefix); it != ctx->arena.end() && it->first.compare(0, strlen(prefix), prefix) == 0; ++it) {
            const uintptr_t b = reinterpret_cast<uintptr_t>(it->second.ptr);
            if (it->second.ptr && a >= b && a < b + it->second.cap) return true;
        }
        return false;
    };
    for (size_t c = 0; c < t.cols.size(); ++c) {
        DevColumn &col = t.cols[c].c;
        if (t.rows == 0 || col.all_null) continue;
        if (col.valid && !mine(col.valid)) {
            uint8_t *v = nullptr;
            FG_TRY(arena_get_t(ctx, node_key(plan, root, "keepn", (int)c).c_str(), (size_t)t.rows + 16, &v));
            FG_HIP(ctx, hipMemcpyAsync(v, col.valid, (size_t)t.rows, hipMemcpyDeviceToDevice, ctx->stream));
            col.valid = v;
        }
        if (col.type == ColType::UTF8) {
            if (mine(col.values) && mine(col.offsets)) continue;
            void *bytes = nullptr;
            int32_t *offs = nullptr;
            FG_TRY(arena_get(ctx, node_key(plan, root, "keepb", (int)c).c_str(), (size_t)col.bytes + 16, &bytes));
            FG_TRY(arena_get_t(ctx, node_key(plan, root, "keepo", (int)c).c_str(), (size_t)t.rows + 4, &offs));
            if (col.bytes) FG_HIP(ctx, hipMemcpyAsync(bytes, col.values, (size_t)col.bytes, hipMemcpyDeviceToDevice, ctx->stream));
            FG_HIP(ctx, hipMemcpyAsync(offs, col.offsets, sizeof(int32_t) * ((size_t)t.rows + 1), hipMemcpyDeviceToDevice, ctx->stream));
            col.values = bytes;
            col.offsets = offs;
        } else {
            if (mine(col.values)) continue;
            void *vals = nullptr;
            FG_TRY(arena_get(ctx, node_key(plan, root, "keepv", (int)c).c_str(), (size_t)t.rows * col_width(col.type) + 16, &vals));
            FG_HIP(ctx, hipMemcpyAsync(vals, col.values, (size_t)t.rows * col_width(col.type), hipMemcpyDeviceToDevice, ctx->stream));
            col.values = vals;
        }
    }
    plan->retained = t;
    plan->has_retained = true;
    if (rows) *rows = t.rows;
    return FLOCKGPU_OK;   // no host wait: the consumer's kernels follow on the same stream
}

int flockgpu_plan_execute_retain(flockgpu_plan *plan, int64_t *rows) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    FG_HIP(ctx, hipSetDevice(ctx->device));
    plan->has_retained = false;
    Exec ex{plan, ctx};
    Table t;
    // a root hash repartition is not computed: which partition a key lands in is unobservable once every partition is handed to
    // the same consumer, and that is the only hand-over this call serves
    FG_TRY(ex.exec(plan->ir.root.get(), &t));
    return keep_result(plan, t, rows);
}

// The collective twin of execute_retain (include/flockgpu_comm.h): the result is hash-partitioned over the ranks of `comm` -- or gathered on
// one of them -- by the library's own all-to-all (comm.hip exchange_table) and what this rank receives becomes the retained result.
int flockgpu_plan_exchange_retain(flockgpu_plan *plan, flockgpu_comm *comm, int gather_rank, uint32_t flags, int64_t *rows) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (rows) *rows = 0;
    // ---- returned at once, before any collective
    FG_TRY(exchange_table_check(ctx, comm, "plan_exchange_retain"));
    const int n = flockgpu_comm_size(comm);
    if (flags & ~FLOCKGPU_EXCHANGE_NO_ROWS) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_exchange_retain: unknown flag bits 0x%x", flags & ~FLOCKGPU_EXCHANGE_NO_ROWS);
    if (gather_rank < -1 || gather_rank >= n) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_exchange_retain: gather_rank %d with %d ranks", gather_rank, n);
    if (plan->async_pending) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_exchange_retain: an asynchronous execute is in flight (flockgpu_plan_wait first)");
    const Node *root = plan->ir.root.get();
    if (gather_rank < 0) {
        if (root->kind != NKind::Repartition || root->hash_cols.empty())
            return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_exchange_retain: rows are placed by the root's hash keys, and the plan's root is no RepartitionExec Hash (pass a gather_rank)");
        if (root->hash_diff)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan_exchange_retain: a HashDiff root gives every distinct key a partition of its own; the ranks of a communicator are no such partitions");
    }
    FG_HIP(ctx, hipSetDevice(ctx->device));
    plan->has_retained = false;
    exchange_phase_begin(comm);
    exchange_phase_mark(ctx, comm, "execute");
    const bool no_rows = (flags & FLOCKGPU_EXCHANGE_NO_ROWS) != 0;
    XTableArgs a;
    {
        char prefix[40];
        snprintf(prefix, sizeof prefix, "plan%p.xchg", (const void *)plan);   // buffers named after the plan: keep_result's mine() rule holds for what arrives
        a.name = prefix;
    }
    a.gather_rank = gather_rank;
    {   // names, types and order of the root schema, and where the rows go
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](const void *p, size_t len) {
            for (size_t i = 0; i < len; ++i) h = (h ^ static_cast<const uint8_t *>(p)[i]) * 1099511628211ull;
        };
        for (const Field &f : root->schema) {
            mix(f.name.data(), f.name.size() + 1);
            const int32_t t[2] = {(int32_t)f.type, f.is_ts ? 1 : 0};
            mix(t, sizeof t);
        }
        const int32_t place[2] = {gather_rank, gather_rank < 0 ? root->hash_cols[0] : -1};
        mix(place, sizeof place);
        a.fingerprint = h;
    }
    Exec ex{plan, ctx};
    Table t, blank;   // blank: what a rank without rows announces -- the schema's columns, empty
    blank.cols.assign(root->schema.size(), TCol{});
    for (size_t c = 0; c < blank.cols.size(); ++c) {
        blank.cols[c].c.type = root->schema[c].type;
        blank.cols[c].c.is_ts = root->schema[c].is_ts;
        blank.cols[c].c.nullable = root->schema[c].nullable;
        blank.cols[c].present = true;
    }
    auto describe = [&](const Table &from, int64_t n_rows) -> int {
        if (from.cols.size() != root->schema.size()) return fail(ctx, FLOCKGPU_ERR_HIP, "plan execute: %zu result columns for a schema of %zu", from.cols.size(), root->schema.size());
        a.cols.clear();
        for (size_t c = 0; c < from.cols.size(); ++c) {
            if (!from.cols[c].present && !from.cols[c].c.all_null) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: output column '%s' was not materialised", root->schema[c].name.c_str());
            a.cols.push_back(from.cols[c].c);
        }
        a.rows = n_rows;
        return FLOCKGPU_OK;
    };
    auto produce = [&]() -> int {
        if (n == 1 || gather_rank >= 0) {   // a root hash repartition is skipped, as execute_retain skips it
            FG_TRY(ex.exec(root, &t));
            return describe(t, t.rows);
        }
        // run_plan's placement with the partition count replaced by the communicator's size; a filter directly below the repartition is
        // composed with the send order (its row list goes into the emit pass), never materialised
        const Node *below = root->in[0].get();
        while (below->kind == NKind::Repartition) below = below->in[0].get();
        const bool compose = below->kind == NKind::Filter && plan->fused[(size_t)below->id].kind == kNone && below->schema.size() == root->schema.size() &&
                             root->in[0]->schema.size() == root->schema.size();
        Table in;
        int32_t *sel = nullptr;
        int64_t n_sel = 0;
        if (compose) FG_TRY(ex.filter_rows(below, &in, &sel, &n_sel));
        else FG_TRY(ex.exec(root->in[0].get(), &in));
        const int64_t n_rows = compose ? n_sel : in.rows;
        FG_TRY(describe(in, n_rows));
        TCol k = in.cols[(size_t)root->hash_cols[0]];
        if (!k.present && !k.c.all_null) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan execute: key column was not materialised");
        int64_t *keys = nullptr;
        if (k.c.all_null) {   // every key NULL: one key
            FG_TRY(arena_get_t(ctx, node_key(plan, root, "xk").c_str(), (size_t)n_rows + 2, &keys));
            FG_HIP(ctx, hipMemsetAsync(keys, 0, sizeof(int64_t) * ((size_t)n_rows + 2), ctx->stream));
        } else {
            if (compose) FG_TRY(take_column(ctx, node_key(plan, root, "xkcol").c_str(), in.cols[(size_t)root->hash_cols[0]].c, sel, n_sel, &k.c));
            if (k.c.type == ColType::UTF8) {
                FG_TRY(arena_get_t(ctx, node_key(plan, root, "xk").c_str(), (size_t)n_rows + 2, &keys));
                FG_TRY(hash_utf8_i64(ctx, k.c, n_rows, keys));
            } else {
                FG_TRY(ex.key_i64(root, k, n_rows, "xk", &keys));
            }
            if (k.c.valid) FG_TRY(replace_invalid_i64(ctx, keys, k.c.valid, n_rows, 0));   // (NULL keys: one key as far as placement goes)
        }
        int32_t *folded = nullptr;
        FG_TRY(arena_get_t(ctx, node_key(plan, root, "xfold").c_str(), (size_t)n_rows + 4, &folded));
        FG_TRY(fold_keys_i32(ctx, keys, n_rows, folded));
        a.keys = folded;
        a.sel = compose ? sel : nullptr;
        return FLOCKGPU_OK;
    };
    int rc = FLOCKGPU_OK;
    if (no_rows) rc = describe(blank, 0);
    else rc = produce();
    if (rc != FLOCKGPU_OK) {   // the failed rank still takes part: the empty table stands in
        const std::string first_error = ctx->last_error;
        (void)describe(blank, 0);
        a.keys = nullptr;
        a.sel = nullptr;
        ctx->last_error = first_error;
    }
    XTableResult res;
    rc = exchange_table(ctx, comm, rc, a, &res);
    if (rc == FLOCKGPU_OK) {
        if (res.passthrough) {
            rc = keep_result(plan, no_rows ? blank : t, rows);
        } else {
            Table got;
            got.rows = res.rows;
            got.cols.assign(res.cols.size(), TCol{});
            for (size_t c = 0; c < res.cols.size(); ++c) {
                got.cols[c].c = res.cols[c];
                got.cols[c].present = true;
            }
            plan->retained = got;
            plan->has_retained = true;
            if (rows) *rows = got.rows;
        }
    }
    exchange_phase_finish(ctx, comm);
    return rc;
}

int flockgpu_plan_execute(flockgpu_plan *plan, struct ArrowSchema *out_schema, struct ArrowArray *out_batch) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    if (!out_schema || !out_batch) return fail(plan->ctx, FLOCKGPU_ERR_INVALID, "plan_execute: null output");
    if (plan->async_pending) return fail(plan->ctx, FLOCKGPU_ERR_INVALID, "plan_execute: an asynchronous execute is in flight (flockgpu_plan_wait first)");
    int n = 0;
    API_CLOCK("execute");
    return run_plan(plan, false, out_schema, out_batch, 1, &n);
}

int flockgpu_plan_execute_partitioned(flockgpu_plan *plan, struct ArrowSchema *out_schema, struct ArrowArray *out_batches, int capacity,
                                      int *n_partitions) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    if (!out_schema || !out_batches || !n_partitions || capacity < 1) return fail(plan->ctx, FLOCKGPU_ERR_INVALID, "plan_execute_partitioned: bad argument");
    if (plan->async_pending) return fail(plan->ctx, FLOCKGPU_ERR_INVALID, "plan_execute_partitioned: an asynchronous execute is in flight (flockgpu_plan_wait first)");
    return run_plan(plan, true, out_schema, out_batches, capacity, n_partitions);
}

// execute on the ctx's worker thread (the reference: one tokio task per plan, context.rs:172-191); the outputs wait in the plan
int flockgpu_plan_execute_async(flockgpu_plan *plan, int partitioned) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (plan->async_pending) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_execute_async: a call is already in flight on this plan");
    const int cap = partitioned && plan->ir.root->kind == NKind::Repartition ? plan->ir.root->n_parts : 1;
    plan->async_batches.assign((size_t)cap, ArrowArray{});
    plan->async_schema = ArrowSchema{};
    plan->async_n = 0;
    FG_TRY(ctx_submit(ctx, [plan, partitioned, cap] {
        return run_plan(plan, partitioned != 0, &plan->async_schema, plan->async_batches.data(), cap, &plan->async_n);
    }));
    plan->async_pending = true;
    ctx->plan_in_flight = plan;
    return FLOCKGPU_OK;
}

int flockgpu_plan_wait(flockgpu_plan *plan, struct ArrowSchema *out_schema, struct ArrowArray *out_batches, int capacity, int *n_partitions) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (!plan->async_pending) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_wait: no asynchronous execute was started on this plan");
    const int rc = ctx_wait(ctx);
    plan->async_pending = false;
    ctx->plan_in_flight = nullptr;
    auto drop = [&] {
        for (int i = 0; i < plan->async_n; ++i)
            if (plan->async_batches[(size_t)i].release) plan->async_batches[(size_t)i].release(&plan->async_batches[(size_t)i]);
        if (plan->async_schema.release) plan->async_schema.release(&plan->async_schema);
    };
    if (rc != FLOCKGPU_OK) {   // (a failed run_plan exports nothing; whatever it did export is released, never leaked)
        drop();
        return rc;
    }
    if (!out_schema || !out_batches || capacity < plan->async_n) {
        drop();
        return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_wait: %d output batches, room for %d", plan->async_n, capacity);
    }
    // (Arrow C Data Interface: a struct is moved by copying it bitwise and marking the source released)
    *out_schema = plan->async_schema;
    plan->async_schema.release = nullptr;
    for (int i = 0; i < plan->async_n; ++i) {
        out_batches[i] = plan->async_batches[(size_t)i];
        plan->async_batches[(size_t)i].release = nullptr;
    }
    if (n_partitions) *n_partitions = plan->async_n;
    return FLOCKGPU_OK;
}

const char *flockgpu_plan_partition_scheme(void) { return kPartitionScheme; }
int flockgpu_plan_check_partition_scheme(const char *scheme) {
    return scheme && !strcmp(scheme, kPartitionScheme) ? FLOCKGPU_OK : FLOCKGPU_ERR_UNSUPPORTED;
}

int flockgpu_host_alloc(size_t bytes, void **out) {
    if (!out) return FLOCKGPU_ERR_INVALID;
    *out = nullptr;
    return hipHostMalloc(out, bytes ? bytes : 64, hipHostMallocDefault) == hipSuccess ? FLOCKGPU_OK : FLOCKGPU_ERR_OOM;
}
int flockgpu_host_free(void *ptr) { return !ptr || hipHostFree(ptr) == hipSuccess ? FLOCKGPU_OK : FLOCKGPU_ERR_HIP; }
int flockgpu_host_register(void *ptr, size_t bytes) {
    if (!ptr || !bytes) return FLOCKGPU_ERR_INVALID;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? FLOCKGPU_OK : FLOCKGPU_ERR_HIP;
}
int flockgpu_host_unregister(void *ptr) { return ptr && hipHostUnregister(ptr) == hipSuccess ? FLOCKGPU_OK : FLOCKGPU_ERR_HIP; }

}  // extern "C"
