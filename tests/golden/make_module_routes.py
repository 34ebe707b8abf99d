#!/usr/bin/env python3
"""Write tests/golden/module_routes.json: which native calls, cache effects, autograd node or refusal every scenario of
tests/helpers/module_routes.py comes to.

    python tests/golden/make_module_routes.py [output path]

Needs the MI355X and the built library.  The committed file was written by the commit BEFORE the module front of nn_conv.py /
diag_conv.py was folded into one path and is the statement of what the modules selected then; tests/test_gpu_module_routes.py
compares today's record with it.  Regenerate it only together with a deliberate change of a routing rule.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.helpers import module_routes      # noqa: E402

if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "module_routes.json")
    rec = module_routes.record_all()
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(rec)} scenarios, {sum(len(r['calls']) for r in rec.values())} native calls, "
          f"{sum('raises' in r for r in rec.values())} refusals")
