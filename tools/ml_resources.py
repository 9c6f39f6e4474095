"""Resource usage of every ml_detect_kernel instantiation, from the compiler's
kernel-resource-usage remarks (a cross-compile: no GPU needed).

    python tools/ml_resources.py            # markdown table on stdout

Exits non-zero if any instantiation uses scratch memory.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from python_5gtoolbox_amd import build  # noqa: E402

MODES = {0: "exhaustive", 1: "subset", 2: "rank-2"}


def main():
    src = os.path.join(build.CSRC, "ldpc5g_ml.hip")
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([build.HIPCC, *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                              "-o", os.path.join(tmp, "ml.o")], capture_output=True, text=True, check=True)
    rows = []
    for blk in re.split(r"remark: [^\n]*Function Name: ", res.stderr)[1:]:
        m = re.match(r"\S*ml_detect_kernelILi(\d)ELi(\d)E15HIP_vector_typeI([df])Lj2EELi(\d)ELi(\d+)ELb([01])E", blk)
        if not m:
            continue
        def g(key):
            return int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
        rows.append((int(m[1]), int(m[2]), "c128" if m[3] == "d" else "c64", int(m[4]), int(m[5]), int(m[6]),
                     g("VGPRs"), g("AGPRs"), g("SGPRs"), g("LDS Size [bytes/block]"),
                     g("ScratchSize [bytes/lane]"), g("Occupancy [waves/SIMD]")))
    rows.sort()
    print("| Nr | NL | storage | search | lanes/RE | ML2 | VGPR | AGPR | SGPR | LDS B | scratch B | waves/SIMD |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r[0]} | {r[1]} | {r[2]} | {MODES[r[3]]} | {r[4]} | {'yes' if r[5] else 'no'} | "
              + " | ".join(str(x) for x in r[6:]) + " |")
    worst = max(r[10] for r in rows)
    print(f"\n{len(rows)} instantiations, max scratch {worst} B/lane", file=sys.stderr)
    return 1 if worst else 0


if __name__ == "__main__":
    sys.exit(main())
