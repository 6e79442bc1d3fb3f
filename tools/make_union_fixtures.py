#!/usr/bin/env python3
"""Writes the two union_exec fixtures under tests/golden/plans/ (union.hpp A-U1..7), in the serde_json dialect of the other fixtures:

  person_activity.json   SELECT person, kind, COUNT(*) FROM (SELECT seller AS person, a_date_time AS t, 'auction' AS kind FROM auction
                                                             UNION ALL SELECT bidder, b_date_time, 'bid' FROM bid) GROUP BY person, kind
                         Final <- CoalesceBatches <- Repartition Hash(person, kind) <- Partial <- Union <- two projections over the scans
  bids_two_ranges.json   SELECT auction AS id FROM bid WHERE price > 9000000 UNION ALL SELECT bidder FROM bid WHERE b_date_time > <t>
                         two filters of ONE relation that read different columns of it: both scans list all four bid columns, one source feeds
                         the first and the second reads the fed one (A-U7)

The fork's serialiser cannot be run here: like tools/make_plan_fixtures.py's plans these are AUTHORED from the grammar of the checked-in fixtures; the
`union_exec` tag with `inputs` follows the naming of every tag seen so far.  The other fixtures are not touched."""
import json
import os

P = 8
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "plans")
TS = {"Timestamp": ["Millisecond", None]}


def field(name, dt, nullable=False):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


BID = [field("auction", "Int32"), field("bidder", "Int32"), field("price", "Int32"), field("b_date_time", TS)]
AUCTION = [field("a_id", "Int32"), field("item_name", "Utf8"), field("description", "Utf8"), field("initial_bid", "Int32"), field("reserve", "Int32"),
           field("a_date_time", TS), field("expires", TS), field("seller", "Int32"), field("category", "Int32")]
BIDS_AFTER_MS = 1_436_918_400_000 + 50_000   # the second branch of bids_two_ranges.json keeps the bids after this instant


def schema(fields, name=None):
    return {"fields": fields, "metadata": {"name": name} if name else {}}


def col(name, index):
    return {"physical_expr": "column", "name": name, "index": index}


def lit(kind, v):
    return {"physical_expr": "literal", "value": {kind: v}}


def binary(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def cast(e, t):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": t}


def memory(fields, projection, name):
    return {"execution_plan": "memory_exec", "schema": schema(fields, name), "projection": projection}


def rr(inp):
    return {"execution_plan": "repartition_exec", "input": inp, "partitioning": {"RoundRobinBatch": P}}


def hashp(inp, exprs):
    return {"execution_plan": "repartition_exec", "input": inp, "partitioning": {"Hash": [exprs, P]}}


def coalesce(inp):
    return {"execution_plan": "coalesce_batches_exec", "input": inp, "target_batch_size": 4096}


def proj(inp, exprs, fields):
    return {"execution_plan": "projection_exec", "expr": [[e, n] for e, n in exprs], "input": inp, "schema": schema(fields)}


def filt(inp, pred):
    return {"execution_plan": "filter_exec", "predicate": pred, "input": inp}


def union(inputs, fields):
    return {"execution_plan": "union_exec", "inputs": inputs, "schema": schema(fields)}


def agg(inp, mode, group, aggrs, in_fields, out_fields):
    return {"execution_plan": "hash_aggregate_exec", "mode": mode, "group_expr": [[e, n] for e, n in group], "aggr_expr": aggrs, "input": inp,
            "input_schema": schema(in_fields), "schema": schema(out_fields), "output_rows": {"metric_type": "Counter", "value": 0}}


def person_activity():
    log = [field("person", "Int32"), field("t", TS), field("kind", "Utf8")]
    auctions = proj(rr(memory(AUCTION, [5, 7], "auction")), [(col("seller", 1), "person"), (col("a_date_time", 0), "t"), (lit("Utf8", "auction"), "kind")], log)
    bids = proj(rr(memory(BID, [1, 3], "bid")), [(col("bidder", 0), "bidder"), (col("b_date_time", 1), "b_date_time"), (lit("Utf8", "bid"), "Utf8(\"bid\")")],
                [field("bidder", "Int32"), field("b_date_time", TS), field("Utf8(\"bid\")", "Utf8")])
    cnt = [{"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)}]
    grp = [(col("person", 0), "person"), (col("kind", 2), "kind")]
    part = [field("person", "Int32"), field("kind", "Utf8"), field("COUNT(UInt8(1))[count]", "UInt64", True)]
    fin = [field("person", "Int32"), field("kind", "Utf8"), field("COUNT(UInt8(1))", "UInt64", True)]
    partial = agg(union([auctions, bids], log), "Partial", grp, cnt, log, part)
    return agg(coalesce(hashp(partial, [col("person", 0), col("kind", 1)])), "FinalPartitioned", [(col("person", 0), "person"), (col("kind", 1), "kind")], cnt, log, fin)


def bids_two_ranges():
    one = [field("id", "Int32")]
    high = proj(coalesce(filt(rr(memory(BID, [0, 1, 2, 3], "bid")), binary(col("price", 2), "Gt", lit("Int32", 9_000_000)))), [(col("auction", 0), "id")], one)
    late = proj(coalesce(filt(rr(memory(BID, [0, 1, 2, 3], "bid")), binary(cast(col("b_date_time", 3), "Int64"), "Gt", lit("Int64", BIDS_AFTER_MS)))),
                [(col("bidder", 1), "bidder")], [field("bidder", "Int32")])
    return union([high, late], one)


def main():
    for name, plan in (("person_activity", person_activity()), ("bids_two_ranges", bids_two_ranges())):
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            json.dump(plan, f, indent=1, sort_keys=True)
            f.write("\n")
    print("wrote person_activity.json, bids_two_ranges.json")


if __name__ == "__main__":
    main()
