#!/usr/bin/env python3
"""bench_full_sort_eval.py: one full-sort evaluation batch, fused ranks against the dense path, on one GPU.

Default shape: B = 4096 rows (the reference's eval_batch_size), N = 100,000 items, H = 64, K = 10.  Timed with device events,
`--rounds` (20) alternating rounds in one process after `--warmup` rounds, medians with min - max:

  fused        ac_tsr_amd.rank.full_sort_ranks: pair scores, sweep, fold (+ the exclusion launch with --history)
  dense        what _full_sort_batch_eval plus the collector do on the GPU (recbole/trainer/trainer.py:926-945,
               recbole/evaluator/collector.py:141-153): torch.matmul -> [B, N] scores, scores[:, 0] = -inf,
               scores[history_index] = -inf (with --history), torch.topk(scores, K), position of the target among the K
  ce_fwd       acattn_full_sort_ce_fwd with exact-fp32 products (mode 0) at the same B, N, H: the same products with a
               soft-max instead of a count -- a record beside the fused call, not a gate

and the peak of torch.cuda.max_memory_allocated above the inputs for fused and dense.  Prints a table and one JSON line.
Measurement helper, not product."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ac_tsr_amd import _lib  # noqa: E402
from ac_tsr_amd import rank as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--history", type=int, default=0, help="history pairs per row (0: the sequential loaders' None)")
    a = ap.parse_args()
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    out = torch.randn(a.B, a.H, generator=g).to(dev)
    table = torch.randn(a.N, a.H, generator=g).to(dev)
    target = torch.randint(1, a.N, (a.B,), generator=g).to(dev)
    hist = None
    if a.history:
        hist = (torch.arange(a.B).repeat_interleave(a.history).to(dev),
                torch.randint(1, a.N, (a.B * a.history,), generator=g).to(dev))
    lib = _lib.load()
    p = _lib.CeProblem()
    p.B, p.N, p.H = a.B, a.N, a.H
    p.out, p.table, p.target = out.data_ptr(), table.data_ptr(), target.data_ptr()
    old_mode = lib.acattn_full_sort_ce_products(0)
    ce_ws = torch.empty(lib.acattn_full_sort_ce_workspace_bytes(C.byref(p)), dtype=torch.uint8, device=dev)
    lse, row_loss = torch.empty(a.B, device=dev), torch.empty(a.B, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused():
        return R.full_sort_ranks(out, table, target, first_item=1, history_index=hist).rank

    def dense():
        scores = torch.matmul(out, table.transpose(0, 1))
        scores[:, 0] = -float("inf")
        if hist is not None:
            scores[hist] = -float("inf")
        idx = torch.topk(scores, a.K, dim=-1).indices
        hit = idx == target[:, None]
        return torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.zeros_like(target, dtype=torch.int64))

    def ce_fwd():
        _lib.check(lib.acattn_full_sort_ce_fwd(C.byref(p), ce_ws.data_ptr(), lse.data_ptr(), row_loss.data_ptr(), stream()),
                   "full_sort_ce_fwd")

    paths = {"fused": fused, "dense": dense, "ce_fwd": ce_fwd}
    times = {k: [] for k in paths}
    peak = {}
    # agreement first: the fused rank is the dense position wherever the positive is in the top K (fp32 ties aside)
    r_f, r_d = fused().long(), dense()
    inside = r_d > 0
    agree = int((r_f[inside] == r_d[inside]).sum()), int(inside.sum())
    for name in ("fused", "dense"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        paths[name]()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    for r in range(a.warmup + a.rounds):
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    lib.acattn_full_sort_ce_products(old_mode)
    res = {"B": a.B, "N": a.N, "H": a.H, "K": a.K, "history_pairs_per_row": a.history, "rounds": a.rounds,
           "ranks_equal_in_top_k": f"{agree[0]}/{agree[1]}"}
    print(f"full-sort evaluation batch: B = {a.B}, N = {a.N}, H = {a.H}, K = {a.K}, history pairs per row = {a.history}, "
          f"{a.rounds} alternating rounds after {a.warmup}")
    for name in paths:
        t = times[name]
        res[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
        mem = f"   peak above inputs {peak[name] / 2 ** 20:9.1f} MiB" if name in peak else ""
        print(f"  {name:7s} median {statistics.median(t):8.3f} ms   (min {min(t):8.3f} - max {max(t):8.3f}){mem}")
    res["peak_bytes_above_inputs"] = peak
    print(f"  fused rank == dense position on {agree[0]} of the {agree[1]} rows whose positive is in the dense top {a.K}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
