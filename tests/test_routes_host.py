"""The Aggregator's routing decisions against the recorded table (tests/golden/routes.json).

Run:  python -m pytest tests/test_routes_host.py -m "not gpu" -q

tests/golden/make_golden_routes.py puts every combination of scheme, opt-in key, condition and
round of stub clients (or host-built wire payloads) to the route predicates, to ``aggregate_grads``
and to ``aggregate_wire``, the first touch of the device replaced by a sentinel, and recorded each
value or refusal before the routing layer was refactored.  The table is recomputed here and must
equal the file case by case; the file is never regenerated to make this pass.  No GPU is needed.
"""
import ast
import json

import pytest

import make_golden_routes as mg


@pytest.fixture(scope="module")
def recorded():
    with open(mg.OUT) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def computed():
    return mg.table()


def _named(tab, rows, cases, fields):
    out = tab["outcomes"]
    return [dict(zip(fields, (out[i] for i in tab[rows][c]))) for c in tab[cases]]


@pytest.mark.parametrize("part,fields,cases", [("grads", mg.GRADS_FIELDS, mg.grads_cases),
                                                ("wire", mg.WIRE_FIELDS, mg.wire_cases)])
def test_every_case_decides_as_recorded(recorded, computed, part, fields, cases):
    assert tuple(recorded[f"{part}_fields"]) == fields
    names = [c[0] for c in cases()]
    want = _named(recorded, f"{part}_rows", f"{part}_cases", fields)
    got = _named(computed, f"{part}_rows", f"{part}_cases", fields)
    assert len(names) == len(want) == len(got)
    bad = [(name, w, g) for name, w, g in zip(names, want, got) if w != g]
    assert not bad, f"{len(bad)} of {len(names)} cases differ, first: {bad[0]}"


def test_the_file_is_what_the_generator_writes(recorded, computed):
    assert computed == recorded
    with open(mg.OUT) as fh:
        assert fh.read() == mg.dumps(computed)


def test_the_grid_is_the_full_product(recorded):
    assert len(mg.SCHEMES) == 9 and len(mg.KEYS) == 6 and len(mg.CONDITIONS) == 7
    assert len(mg.client_rounds()) == 15
    assert len(recorded["grads_cases"]) == 9 * 6 * 7 * 15
    assert len(recorded["wire_cases"]) == 9 * 6 * 7 * len(mg.payload_rounds())
    seen = {f: set() for f in mg.GRADS_FIELDS}
    for row in _named(recorded, "grads_rows", "grads_cases", mg.GRADS_FIELDS):
        for f, v in row.items():
            seen[f].add(v)
    # every answer a predicate has, every packet route and the device all occur
    assert {"True", "False"} <= seen["sign_route"] & seen["sign_gram_route"] & seen["sign_trim_route"]
    assert {"100", "not wanted"} <= seen["gram_route_k"] and {"100", "None"} <= seen["ef_batch_k"]
    assert mg.DEVICE in seen["aggregate_grads"] and seen["agg_path"] == {"None"}
    wire = _named(recorded, "wire_rows", "wire_cases", mg.WIRE_FIELDS)
    assert {r["agg_path"] for r in wire} == {"None", "'wire-sign'", "'wire-sign-gram'", "'wire-sign-trim'"}


def test_round_route_is_the_recorded_decision(recorded):
    """``round_route`` raises what ``aggregate_grads`` raised and otherwise names the route the
    recorded predicates give: sign-gram, sign-trim, gram, sign, ef-batch, in that order."""
    from openmsftl_amd import aggregation as ag
    want = _named(recorded, "grads_rows", "grads_cases", mg.GRADS_FIELDS)
    routes = set()
    for (name, scheme, key, cond, clients), rec in zip(mg.grads_cases(), want):
        agg = mg._aggregator(scheme, key, cond, len(clients))
        got = mg._outcome(ag.round_route, agg, clients)
        if rec["aggregate_grads"] != mg.DEVICE:
            assert got == rec["aggregate_grads"], name
            continue
        if rec["sign_gram_route"] == "True":
            expect = ("sign-gram", None)
        elif rec["sign_trim_route"] == "True":
            expect = ("sign-trim", None)
        elif rec["gram_route_k"] != "not wanted":
            expect = ("gram", int(rec["gram_route_k"]))
        elif rec["sign_route"] == "True":
            expect = ("sign", None)
        elif rec["ef_batch_k"] != "None":
            expect = ("ef-batch", int(rec["ef_batch_k"]))
        else:
            expect = None
        assert ast.literal_eval(got) == expect, name
        assert agg.agg_path is None, name
        routes.add(expect and expect[0])
    assert routes == {None, "gram", "sign-gram", "sign-trim", "sign", "ef-batch"}
