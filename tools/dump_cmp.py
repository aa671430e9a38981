#!/usr/bin/env python3
"""dump_cmp.py <dir A> <dir B> [top]: compares two `bench.py --dump-outputs` directories array by array.
Prints the number of arrays, how many are bitwise equal, the `top` (default 12) largest differences as
rel = max|a - b| / max|a|, and the scalar losses of both sides.  Measurement helper, not product."""
import glob
import os
import sys

import numpy as np

a_dir, b_dir = sys.argv[1], sys.argv[2]
top = int(sys.argv[3]) if len(sys.argv) > 3 else 12
names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a_dir, "*.npy")))
missing = [n for n in names if not os.path.exists(os.path.join(b_dir, n))]
assert names and not missing, f"arrays missing in {b_dir}: {missing[:5]}"
rows, equal, losses = [], 0, []
for n in names:
    a, b = np.load(os.path.join(a_dir, n)), np.load(os.path.join(b_dir, n))
    assert a.shape == b.shape, n
    if a.ndim == 0:
        losses.append(f"  {n}: {a!r} / {b!r}")
    if a.tobytes() == b.tobytes():
        equal += 1
        continue
    d = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    s = float(np.abs(a.astype(np.float64)).max())
    rows.append((d / s if s > 0 else float("inf"), d, s, n))
rows.sort(reverse=True)
print(f"{len(names)} arrays, bitwise equal: {equal}")
for rel, d, s, n in rows[:top]:
    print(f"  rel {rel:.3e}  abs {d:.3e}  scale {s:.3e}  {n}")
print("\n".join(losses))
