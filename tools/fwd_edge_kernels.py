#!/usr/bin/env python3
"""fwd_edge_kernels.py <trace dir> [out]: which forward kernel each case of tests/_fwd_edge_cases.py ran.

Input: the *kernel_trace.csv of ONE process that ran tests/test_hip_fwd_edges.py in table order under
`rocprofv3 --kernel-trace --output-format csv` (a run of its own, the program after `--`, under a time limit; only after the
module is green: this is a coverage record).  Every case launches the forward twice, so the forward kernels of the trace,
in dispatch order, pair up with the cases.  Writes the table `case id -> kernel<template arguments>` (profiles/
fwd_edge_kernels.txt) and fails where a kernel is not the form tests/_fwd_edge_cases.py::expected_form gives."""
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _fwd_edge_cases as E  # noqa: E402

KERNEL = re.compile(r"(acattn_long_fwd_kernel|acattn_fwd_stream_kernel|acattn_fwd_dma_kernel|acattn_fwd_fast_kernel|acattn_fwd_kernel)(<[^>]*>)")
FORM = {"acattn_long_fwd_kernel": "long", "acattn_fwd_dma_kernel": "dma", "acattn_fwd_fast_kernel": "fast", "acattn_fwd_kernel": "general"}


def form_of(name, args):
    if name == "acattn_fwd_stream_kernel":
        return "stream4" if args.strip("<>").split(",")[1].strip() == "4" else "stream13"
    return FORM[name]


def main(argv):
    paths = sorted(glob.glob(os.path.join(argv[1], "**", "*kernel_trace.csv"), recursive=True))
    assert len(paths) == 1, f"one process, one trace: {paths}"
    with open(paths[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    names = [r["Kernel_Name"] for r in rows]
    if any(n.startswith("_Z") for n in names):  # a trace with mangled names
        import subprocess
        names = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    fwd = [m.groups() for m in (KERNEL.search(n) for n in names) if m]
    assert len(fwd) == 2 * len(E.CASES), f"{len(fwd)} forward launches for {len(E.CASES)} cases"
    lines, bad, seen = [], [], set()
    for n, c in enumerate(E.CASES):
        (name, args), second = fwd[2 * n], fwd[2 * n + 1]
        note = ""
        if E.tail_block(c):
            note = f"  tail block, {c.L % 16} row(s), nT = {(c.L + 15) // 16}" + (", grid re-ordered" if E.reordered_grid(c) else "")
        lines.append(f"{c.id:<64} {name}{args}{note}")
        seen.add(name + args)
        if (name, args) != second or form_of(name, args) != E.expected_form(c) or form_of(name, args) != c.form:
            bad.append(f"{c.id}: {name}{args} / {second[0]}{second[1]}, expected {E.expected_form(c)}")
    out = [f"# {len(E.CASES)} cases, {len(seen)} distinct kernel instantiations; every case launched the same kernel twice",
           "# (the tail block is a path inside acattn_fwd_stream_kernel<DH, 4, .., PRE = true>, marked from the case's length)", ""]
    out += lines + ["", "# distinct instantiations"] + sorted(seen)
    text = "\n".join(out) + "\n"
    if len(argv) > 2:
        with open(argv[2], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    assert not bad, "\n".join(bad)


if __name__ == "__main__":
    main(sys.argv)
