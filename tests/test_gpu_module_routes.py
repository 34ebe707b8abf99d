"""GPU tier: WHICH regime a call of the modules takes (every regime has parity tests, nothing pinned the
selection).  tests/golden/module_routes.json holds, for every scenario of tests/helpers/module_routes.py, the ordered native calls
with their arguments, the change of the cache counters, the autograd node of each output and - for a call that must refuse - the
exception's type and text, as the modules behaved before their front was folded into one path (tests/golden/make_module_routes.py).
Each scenario is run again here and must come to the same record."""
import json
import os

import pytest
import torch

from tests.helpers import module_routes

pytestmark = pytest.mark.gpu
RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "module_routes.json")))


@pytest.fixture(scope="module")
def table():
    assert torch.cuda.is_available(), "GPU tier needs an MI355X"
    return module_routes.scenarios()


def test_the_record_covers_the_table(table):
    assert sorted(table) == sorted(RECORD)


@pytest.mark.parametrize("sid", sorted(RECORD))
def test_scenario_takes_the_recorded_route(table, sid):
    got = json.loads(json.dumps(module_routes.run(sid, table)[0]))
    want = RECORD[sid]
    assert got.get("raises") == want.get("raises")
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    assert got == want
