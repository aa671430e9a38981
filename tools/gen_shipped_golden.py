#!/usr/bin/env python3
"""Generate the fixtures `model_yelp` and `model_sports` under tests/golden/ by RUNNING THE GENUINE REFERENCE at the shape
of its yelp and amazon-sports-outdoors / amazon-toys-games configurations (hidden 128, inner 64; 3 layers of 8 heads, 2 layers
of 2 heads), the way oracle/gen_golden.py makes model_beauty.npz: the module is imported unchanged and its `model_case`
called twice.  While generating, each case is also evaluated with the CPU restatement (oracle/ac_tsr_ref.py) and the run
aborts if the two disagree.

TEST INFRASTRUCTURE ONLY; copies nothing from the reference, only tensors are written.

New files in this repository stay under 1 MiB each (MAX_BYTES), and at hidden 128 the parameters and their gradients alone
are 3 MB.  So a case is written as tests/golden/<name>.partNN.npz: the arrays `model_case` saved, untouched, under their
own keys, dealt out in key order over as many compressed files as it takes.  tests/test_hip_shipped_configs.py puts the
parts of a case together again into one <name>.npz that tests/_golden.py `Case` loads.

Usage:  ACTSR_REFERENCE=<checkout of the reference> python tools/gen_shipped_golden.py
"""
import glob
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20
PART_PAYLOAD = 900 * 1024  # uncompressed array bytes per part: the zip directory and the headers fit in the rest

# name -> arguments of oracle.gen_golden.model_case
CASES = {
    "model_yelp": dict(B=6, L=50, H=128, h=8, inner=64, n_layers=3, n_items=400, seed=21, sigma=0.05, train=False),
    "model_sports": dict(B=6, L=50, H=128, h=2, inner=64, n_layers=2, n_items=400, seed=22, sigma=0.05, train=True),
}


def write_parts(name, arrays):
    for old in glob.glob(os.path.join(GOLDEN, name + ".part*.npz")):
        os.remove(old)
    parts, size = [{}], 0
    for key in sorted(arrays):
        n = arrays[key].nbytes
        if parts[-1] and size + n > PART_PAYLOAD:
            parts.append({})
            size = 0
        parts[-1][key] = arrays[key]
        size += n
    for k, part in enumerate(parts):
        path = os.path.join(GOLDEN, f"{name}.part{k:02d}.npz")
        np.savez_compressed(path, **part)
        nbytes = os.path.getsize(path)
        if nbytes >= MAX_BYTES:
            raise SystemExit(f"{path}: {nbytes} bytes, not under {MAX_BYTES}")
        print(f"  wrote tests/golden/{os.path.basename(path)}  ({len(part)} arrays, {nbytes} bytes)")


def main():
    ref = os.environ.get("ACTSR_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref or not os.path.isdir(os.path.join(ref, "recbole")):
        raise SystemExit("usage: ACTSR_REFERENCE=<checkout of the reference> python tools/gen_shipped_golden.py  (or pass the path)")
    os.environ["ACTSR_REFERENCE"] = ref
    from oracle import gen_golden  # imports the reference
    with tempfile.TemporaryDirectory() as whole:
        gen_golden.OUT = whole  # model_case saves one <name>.npz there
        for name, args in CASES.items():
            gen_golden.model_case(name, **args)
            z = np.load(os.path.join(whole, name + ".npz"), allow_pickle=False)
            write_parts(name, {k: z[k] for k in z.files})


if __name__ == "__main__":
    main()
