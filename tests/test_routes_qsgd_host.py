"""The routing of QSGD clients and payloads against the recorded table (tests/golden/routes_qsgd.json).

Run:  python -m pytest tests/test_routes_qsgd_host.py -m "not gpu" -q

tests/golden/make_golden_routes_qsgd.py puts every combination of scheme, ``qsgd_packets``,
condition and round of stub QSGD clients (or host-built payloads that hold a QSGD packet) to
``qsgd_route`` and ``round_route`` and to ``aggregate_wire``, the first touch of the device replaced
by a sentinel, and recorded each value or refusal before aggregate_wire's payload kinds were given
one layer.  The table is recomputed here and must equal the file case by case; the file is never
regenerated to make this pass.  No GPU is needed.
"""
import json
import re

import pytest

import make_golden_routes as mg
import make_golden_routes_qsgd as mq


def _named(tab, rows, cases, fields):
    out = tab["outcomes"]
    return [dict(zip(fields, (out[i] for i in tab[rows][c]))) for c in tab[cases]]


@pytest.fixture(scope="module")
def recorded():
    with open(mq.OUT) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def computed():
    return mq.table()


@pytest.mark.parametrize("part,fields,cases", [("grads", mq.GRADS_FIELDS, mq.grads_cases),
                                                ("wire", mq.WIRE_FIELDS, mq.wire_cases)])
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
    with open(mq.OUT) as fh:
        assert fh.read() == mq.dumps(computed)


def test_the_grid_is_the_full_product_and_every_outcome_class_occurs(recorded):
    assert mq.SCHEMES is mg.SCHEMES and mq.CONDITIONS is mg.CONDITIONS
    assert len(mq.SCHEMES) == 9 and len(mq.KEYS) == 2 and len(mq.CONDITIONS) == 7
    assert len(mq.client_rounds()) == 9 and len(mq.payload_rounds()) == 9
    assert len(recorded["grads_cases"]) == 9 * 2 * 7 * 9
    assert len(recorded["wire_cases"]) == 9 * 2 * 7 * 9
    names = [c[0] for c in mq.grads_cases()]
    assert "fed_avg+pc | qsgd_packets | none | one width" in names     # qsgd_packets with pc_analysis "gram"
    grads = _named(recorded, "grads_rows", "grads_cases", mq.GRADS_FIELDS)
    by_name = dict(zip(names, grads))
    assert by_name["fed_avg | qsgd_packets | none | one width"] == {"qsgd_route": "True",
                                                                    "round_route": "('qsgd', None)"}
    assert by_name["fed_avg | none | none | one width"] == {"qsgd_route": "False", "round_route": "None"}
    assert by_name["fed_avg+pc | qsgd_packets | none | one width"]["qsgd_route"] == "False"
    assert {r["qsgd_route"] for r in grads} == {"True", "False"}
    wire = _named(recorded, "wire_rows", "wire_cases", mq.WIRE_FIELDS)
    assert {r["agg_path"] for r in wire} == {"None", "'wire-qsgd'"}
    outcomes = {r["aggregate_wire"] for r in wire}
    assert any(r["aggregate_wire"] == mq.DEVICE and r["agg_path"] == "'wire-qsgd'" for r in wire)
    for must in ("NotImplementedError: .*mixes QSGD packets", "NotImplementedError: .*fed_avg for QSGD packets",
                 "ValueError: payload 1: qsgd wire: .*level 5 above s = 4", "NotImplementedError: .*one length n"):
        assert any(re.match(must, o) for o in outcomes), must
