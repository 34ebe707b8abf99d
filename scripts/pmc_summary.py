#!/usr/bin/env python3
"""Reduce rocprofv3 counter runs of the headline forward kernel (scripts/gpu/fwd_shape_ab.sh) to one line per run:

    python scripts/pmc_summary.py DIR TAG [TAG ...]      # reads DIR/pmc_TAG/**/*counter_collection.csv + *kernel_trace.csv

Per dispatch of gpde_fused_f16v6_kernel the counter values are summed over their instances and the duration is taken from
the kernel trace; the line gives the averages over the dispatches and, where the counters are there, the effective clock
(GRBM_GUI_ACTIVE / 8 XCDs / duration), the matrix-pipe share (SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE x 128)) and the
LDS bank-conflict share (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE)."""
import csv
import glob
import os
import sys
from collections import defaultdict

KERNEL = "gpde_fused_f16v6_kernel"


def summary(d):
    cf = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
    kf = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not cf or not kf:
        return None
    dur = {}
    for r in csv.DictReader(open(kf[0])):
        if KERNEL in r["Kernel_Name"]:
            dur[r["Dispatch_Id"]] = (float(r["End_Timestamp"]) - float(r["Start_Timestamp"])) / 1e6
    ctr = defaultdict(lambda: defaultdict(float))
    for r in csv.DictReader(open(cf[0])):
        if KERNEL in r["Kernel_Name"]:
            ctr[r["Dispatch_Id"]][r["Counter_Name"]] += float(r["Counter_Value"])
    ids = [k for k in ctr if k in dur]
    if not ids:
        return None
    out = {"dispatches": len(ids), "ms": sum(dur[k] for k in ids) / len(ids)}
    for name in sorted({n for k in ids for n in ctr[k]}):
        out[name] = sum(ctr[k][name] for k in ids) / len(ids)
    return out


def main():
    base = sys.argv[1]
    for tag in sys.argv[2:]:
        s = summary(os.path.join(base, f"pmc_{tag}"))
        if s is None:
            print(f"{tag}: no counter table")
            continue
        parts = [f"{tag}: {s['dispatches']} dispatches, {s['ms']:.2f} ms under the profiler"]
        ga = s.get("GRBM_GUI_ACTIVE")
        if ga:
            parts.append(f"effective clock {ga / 8 / (s['ms'] * 1e-3) / 1e9:.3f} GHz")
            if s.get("SQ_VALU_MFMA_BUSY_CYCLES"):
                parts.append(f"matrix pipe busy {100 * s['SQ_VALU_MFMA_BUSY_CYCLES'] / (ga * 128):.1f} %")
        if s.get("SQ_LDS_IDX_ACTIVE"):
            parts.append(f"LDS bank conflict / active {100 * s.get('SQ_LDS_BANK_CONFLICT', 0.0) / s['SQ_LDS_IDX_ACTIVE']:.2f} %")
        parts.append(" ".join(f"{k}={v:.4g}" for k, v in s.items() if k not in ("dispatches", "ms")))
        print(", ".join(parts))


if __name__ == "__main__":
    main()
