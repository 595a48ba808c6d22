"""Compare two gfx950 assembly listings of one HIP source kernel by kernel.

    hipcc -x hip --offload-arch=gfx950 --cuda-device-only -S -O3 ... mlp_step3.hip -o parent.s   (parent commit)
    hipcc ... mlp_step3.hip -o branch.s                                                       (this tree)
    python scripts/asm_kernel_diff.py parent.s branch.s [--match mlp3_one_kernel]

For every kernel symbol it prints whether the instruction stream (labels and comments
dropped, so a renumbered basic block does not count) is identical in both listings, and
a resource table (VGPR / AGPR / SGPR / LDS / scratch / spills) taken from the listing's
``.amdhsa_`` directives and its trailing comments.  Exit status 1 when a kernel selected
by ``--match`` differs or exists on one side only.
"""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
from typing import Dict, List, Tuple

_RES = {
    "vgpr": re.compile(r";\s*NumVgprs:\s*(\d+)"),
    "agpr": re.compile(r";\s*NumAgprs:\s*(\d+)"),
    "sgpr": re.compile(r";\s*TotalNumSgprs:\s*(\d+)"),
    "lds": re.compile(r";\s*LDSByteSize:\s*(\d+)"),
    "scratch": re.compile(r";\s*ScratchSize:\s*(\d+)"),
    "occupancy": re.compile(r";\s*Occupancy:\s*(\d+)"),
}
_LABEL = re.compile(r"^\.?[A-Za-z_$][\w$.]*:")
_BBREF = re.compile(r"\.LBB\d+_\d+")


def kernels(path: str) -> Dict[str, Tuple[List[str], Dict[str, int]]]:
    """name -> (instruction lines, resources) for every ``.type name,@function`` kernel."""
    out: Dict[str, Tuple[List[str], Dict[str, int]]] = {}
    name, ins, res, in_code = None, [], {}, False
    with open(path) as f:
        for raw in f:
            line = raw.rstrip("\n")
            m = re.match(r"\s*\.type\s+(\S+),@function", line)
            if m:
                name, ins, res, in_code = m.group(1), [], {}, True
                out[name] = (ins, res)
                continue
            if name is None:
                continue
            if in_code and re.match(r"\s*\.section\s+\.rodata", line):
                in_code = False
            # the resource comments follow the kernel descriptor, before the next .type
            for k, rx in _RES.items():
                mm = rx.search(line)
                if mm and k not in res:
                    res[k] = int(mm.group(1))
            if not in_code:
                continue
            code = line.split(";", 1)[0].strip()
            if not code or _LABEL.match(code) or code.startswith("."):
                continue
            # block labels are numbered per function index, which shifts when kernels are added
            ins.append(_BBREF.sub(".LBB", code))
    _spills(path, out)
    return out


def _spills(path: str, out) -> None:
    """sgpr_spill / vgpr_spill of every kernel from the code object metadata at the listing's end."""
    cur: Dict[str, int] = {}
    sym = None
    in_meta = False

    def flush():
        if sym in out:
            out[sym][1].update(cur)

    with open(path) as f:
        for line in f:
            if ".amdgpu_metadata" in line:
                in_meta = not line.lstrip().startswith(".end_amdgpu_metadata")
                continue
            if not in_meta:
                continue
            if re.match(r"\s*-\s+\.", line):  # the next kernel's entry
                flush()
                cur, sym = {}, None
            m = re.search(r"\.(sgpr|vgpr)_spill_count:\s*(\d+)", line)
            if m:
                cur[m.group(1) + "_spill"] = int(m.group(2))
            m = re.search(r"\.symbol:\s*'?([^'\s]+?)\.kd'?\s*$", line)
            if m:
                sym = m.group(1)
    flush()


def demangle(names: List[str]) -> Dict[str, str]:
    try:
        p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, p.stdout.splitlines()))
    except Exception:  # noqa: BLE001
        return {n: n for n in names}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--match", default="mlp3_one_kernel", help="kernels that must be identical (substring)")
    ap.add_argument("--table", default="mlp3_", help="kernels listed in the resource table (substring)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="rewrite demangled names before pairing (a kernel that gained a defaulted "
                         "template or trailing argument keeps its partner)")
    a = ap.parse_args()

    def keyed(ks):
        dm = demangle(sorted(ks))
        out = {}
        for n, v in ks.items():
            k = dm[n]
            for r in a.rename:
                old, new = r.split("=", 1)
                k = k.replace(old, new)
            out[k] = v
        return out

    kp, kb = keyed(kernels(a.parent)), keyed(kernels(a.branch))
    names = sorted(set(kp) | set(kb))
    pretty = {n: n for n in names}
    bad = 0
    print("== instruction streams, parent vs branch ==")
    for n in names:
        if n in kp and n in kb:
            same = kp[n][0] == kb[n][0]
            state = f"identical ({len(kp[n][0])} instructions)" if same else \
                f"DIFFERENT ({len(kp[n][0])} vs {len(kb[n][0])} instructions)"
        else:
            same = False
            state = "only in parent" if n in kp else "only in branch (new)"
        if a.match in n and not same:
            bad += 1
        print(f"{state:42s} {pretty[n]}")
    print()
    print("== resources (branch) ==")
    cols = ["vgpr", "agpr", "sgpr", "lds", "scratch", "sgpr_spill", "vgpr_spill", "occupancy"]
    print(" ".join(f"{c:>10s}" for c in cols) + "  kernel")
    for n in names:
        if n not in kb or a.table not in n:
            continue
        r = kb[n][1]
        print(" ".join(f"{r.get(c, -1):>10d}" for c in cols) + f"  {pretty[n]}")
    print()
    print(f"kernels matching {a.match!r} that differ: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
