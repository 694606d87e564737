"""The batch plan routes every batch of the route table (tests/routes.py) as the commit before it
did: kernel id, staged or not, workspace bytes, row by row against tests/golden/routes.json. No
kernel is launched; the queries upload (and compile) the table's programs."""
import json

import pytest

import routes


@pytest.mark.gpu
def test_routes_match_recorded(cuda):
    with open(routes.FIXTURE) as f:
        golden = json.load(f)
    table = routes.table()
    assert [name for name, _, _ in table] == list(golden["rows"]), "the table and the fixture differ"
    asker = routes.Asker(cuda.index)
    same_cus = asker.cus == golden["cus"]
    bad = []
    for name, prog, kw in table:
        got, want = asker.ask(prog, kw), golden["rows"][name]
        for field, g, w in zip(("kernel", "staged", "workspace_bytes"), got, want):
            # (a tier-1 batch's wave slots are sized by the device's CU count)
            if field == "workspace_bytes" and not same_cus and \
                    (asker.progs[prog].tier == 1 or kw.get("init_fp")):
                continue
            if g != w:
                bad.append(f"{name}: {field} {g}, recorded {w}")
    assert not bad, "\n".join(bad[:40])
