"""Per-gap census of an MFMA loop in hipcc's device assembly: how many non-MFMA instructions ride behind each MFMA.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I graph-pde_amd/csrc --cuda-device-only -S -o v6.s graph-pde_amd/csrc/gpde_fused_f16v6.hip
    python scripts/mfma_gap_census.py v6.s gpde_fused_f16v6_kernelILi0ELb0E [min_mfmas]

For every basic block of the named function with at least min_mfmas (default 90) MFMAs it prints one row: per gap the
number of vector / LDS / vector-memory instructions and s_nop pads (the instructions that compete with the MFMA for the
SIMD's issue port; scalar ALU is counted apart), then the totals by class and the MFMAs whose D is not their C."""
import re
import sys


def census(path, func, min_mfmas=90):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_]\S*:", l) and func in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur, name = [], [], lines[start].split(":")[0]
    for l in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            blocks.append((name, cur))
            name, cur = m.group(1), []
            continue
        t = l.strip()
        if not t or t.startswith((";", ".", "//")):
            continue
        cur.append(t.split(";")[0].strip())
    blocks.append((name, cur))
    out = []
    for name, ins in blocks:
        n_mfma = sum(i.startswith("v_mfma") for i in ins)
        if n_mfma < min_mfmas:
            continue
        gaps, cls, salu, d_ne_c = [], {"valu": 0, "lds": 0, "vmem": 0, "nop": 0, "accvgpr": 0, "lane": 0}, 0, 0
        seen = False
        for i in ins:
            op = i.split()[0]
            if op.startswith("v_mfma"):
                seen = True
                gaps.append(0)
                regs = [r.strip() for r in i[len(op):].split(",")]
                if len(regs) >= 4 and regs[3].split()[0] not in (regs[0], "0"):
                    d_ne_c += 1
                continue
            if not seen:
                continue
            if op.startswith("v_accvgpr"):
                k = "accvgpr"
            elif op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
                k = "lane"
            elif op.startswith("v_"):
                k = "valu"
            elif op.startswith("ds_"):
                k = "lds"
            elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
                k = "vmem"
            elif op == "s_nop":
                k = "nop"
            else:
                salu += 1
                continue
            cls[k] += 1
            gaps[-1] += 1
        out.append((name, n_mfma, gaps, cls, salu, d_ne_c))
    return out


if __name__ == "__main__":
    mn = int(sys.argv[3]) if len(sys.argv) > 3 else 90
    for name, n_mfma, gaps, cls, salu, d_ne_c in census(sys.argv[1], sys.argv[2], mn):
        print(f"{name}: {n_mfma} MFMAs, {sum(g == 0 for g in gaps)} empty gaps, most in one gap {max(gaps)}, "
              f"gaps over 2: {sum(g > 2 for g in gaps)}, D != C on {d_ne_c} MFMAs, scalar {salu}, " +
              " ".join(f"{k} {v}" for k, v in cls.items()))
        print("  " + " ".join(str(g) for g in gaps))
