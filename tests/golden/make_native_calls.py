#!/usr/bin/env python3
"""Write tests/golden/native_calls_w64.json: what every form of tests/helpers/native_recorder.py hands to libgpde.so.

    python tests/golden/make_native_calls.py [--new-only] [output path]

Host only (no GPU, no library).  The committed file was written by the commit BEFORE the 64-wide wrappers of ops.py were given
one forward body and shared backward helpers, and is the statement of what they passed on then; tests/test_native_calls_host.py
compares today's record with it.  Regenerate it only together with a deliberate change of a native call.  `--new-only` keeps
every entry the file already holds as it is and records only the forms it lacks: the way to bring further wrappers under the
record BEFORE they are touched (the edge-weight wrappers' entries were written so, ahead of the one backward body).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.helpers import native_recorder      # noqa: E402

if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a != "--new-only"]
    path = argv[0] if argv else os.path.join(HERE, "native_calls_w64.json")
    if "--new-only" in sys.argv[1:]:
        with open(path) as f:
            rec = json.load(f)
        rec.update({f[0]: native_recorder.record(f) for f in native_recorder.forms() if f[0] not in rec})
    else:
        rec = native_recorder.record_all()
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(rec)} forms, {sum(len(r['calls']) for r in rec.values())} calls")
