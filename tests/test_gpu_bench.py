"""GPU tier: a plain `bench.py` run measures its headline figure and nothing else - every other leg (CPU baseline, the other
precision, node-table attributes, MGKN, depth reuse, backward, in-run traffic, the next sample's attribute reorder) is
`--full`'s.  Run as its own process, as the benchmark is run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_measures_the_headline_alone(tmp_path):
    detail = tmp_path / "detail.json"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "g16",
           "--detail-out", str(detail)]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "M-edges/s through fused NNConv fwd (width=64)" and line["unit"] == "M-edges/s"
    assert line["higher_is_better"] is True and line["dtype"].startswith("f32")
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["roofline"]["launches_per_step"] >= 1                    # from the timed steps' own launches
    assert line["rel_l2_sample"] is None and line["cpu_baseline"] is None
    assert line["summary"]["graph_prep_ms"]["attr_reorder_next_sample_ms"] is None
    assert [k for k, v in line["summary"].items() if v is not None] == ["graph_prep_ms", "mgkn_keys"]
    d = json.loads(detail.read_text())
    for leg in ("alt_precision", "node_table_attributes", "cpu_baseline", "mgkn", "depth_reuse", "backward"):
        assert d[leg] is None, leg
