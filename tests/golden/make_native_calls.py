#!/usr/bin/env python3
"""Write tests/golden/native_calls_w64.json: what every form of tests/helpers/native_recorder.py hands to libgpde.so.

    python tests/golden/make_native_calls.py [output path]

Host only (no GPU, no library).  The committed file was written by the commit BEFORE the 64-wide wrappers of ops.py were given
one forward body and shared backward helpers, and is the statement of what they passed on then; tests/test_native_calls_host.py
compares today's record with it.  Regenerate it only together with a deliberate change of a native call.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.helpers import native_recorder      # noqa: E402

if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "native_calls_w64.json")
    rec = native_recorder.record_all()
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(rec)} forms, {sum(len(r['calls']) for r in rec.values())} calls")
