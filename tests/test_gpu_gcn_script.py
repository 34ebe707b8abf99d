"""GPU tier: the reference's GCN baseline script, byte for byte (multipole-graph-neural-operator/neurips4_GCN.py), on the native
GCNConv and on the stock-torch composite of tests/helpers/composite_gcn.py, from the same seed - the numbers it prints must agree.

The script is looked up like the others (tests/test_gpu_reference_scripts.py); when it is not staged the test skips.  Overrides,
through the runner's line tracer: ntrain=2 (ntrain=1 would make UnitGaussianNormalizer's std NaN), ntest=1, epochs=2, r=20 - the
tracer re-imposes `r` before `s` is derived from it, so the run is at s = 22 (484 nodes).  Every printed number is downstream of an
Adam step (two steps per epoch), which is REL_LATER of that file."""
import math

import pytest

from tests.test_gpu_reference_scripts import REL_LATER, _have, _run

pytestmark = pytest.mark.gpu
NAME = "neurips4_GCN.py"
SETS = ["ntrain=2", "ntest=1", "epochs=2", "r=20"]


def _numbers(out):
    vals = []
    for line in out.split("[run_reference_script]")[0].splitlines():
        t = line.split()
        if "[" in line or not t or not t[0].isdigit():
            continue
        try:
            if len(t) == 4:
                vals += [float(t[2]), float(t[3])]          # epoch: train mse, train l2 (t[1] = seconds)
            elif len(t) == 3:
                vals.append(float(t[2]))                    # test epoch: test l2
        except ValueError:
            pass
    return vals


@pytest.mark.skipif(not _have(NAME), reason="reference scripts not staged on this box")
def test_gcn_baseline_script_runs_unchanged():
    out = _run(NAME, SETS)
    assert "resolution 22" in out, out[-1500:]
    native = _numbers(out)
    assert len(native) == 2 * 2 + 1 and all(math.isfinite(v) for v in native), (native, out[-1500:])
    out_c = _run(NAME, SETS, composite=True)
    composite = _numbers(out_c)
    assert len(composite) == len(native)
    print(NAME, "native", native, "composite", composite)
    for k, (a, b) in enumerate(zip(native, composite)):
        assert math.isfinite(b) and abs(a - b) <= REL_LATER * abs(b), (k, a, b, native, composite)
