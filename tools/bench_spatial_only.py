#!/usr/bin/env python3
"""bench_spatial_only.py: what the spatial-only configuration (BASELINE configuration 2) costs on the MI355X.

(a) kernel level, at B=512 L=50 H=64 2 heads and B=512 L=200 H=128 4 heads, p_drop 0.5, item_length ~ U{1..L}:
      spatial_fwd        acattn_calibrated_attention_fwd with adversarial = 0 (affine planes given, as the layer runs it)
      spatial_bwd        acattn_spatial_attention_bwd (the row kernel + the key kernel + the zero fill of the partials)
      adversarial_bwd_*  acattn_calibrated_attention_bwd with BOTH context cotangents, pinned to the streaming pair
                         (ACATTN_BWD_STREAM) and auto-dispatched (row-resident at L <= 64)
    each over >= 5 rotating buffer sets (working set beyond the 256 MB Infinity Cache), >= 200 launches between two
    device events, median of the rounds;
(b) step level: the hipGraph-captured train_step of a 2-layer ACSASRec with adversarial_calibrator=False beside the full
    AC-SASRec step (100k items, B=512, L=50), medians of per-step device-event times.

Prints ONE JSON line.  Measurement helper, not product; needs the GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ac_tsr_amd as A  # noqa: E402
from ac_tsr_amd import _lib  # noqa: E402

DEV = "cuda"


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _time(launch, nsets, iters, rounds):
    """Median over `rounds` of (device time of `iters` launches) / iters, in microseconds."""
    for i in range(min(20, iters)):
        launch(i % nsets)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(rounds):
        e0.record()
        for i in range(iters):
            launch(i % nsets)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return {"us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def kernel_level(B, L, H, nh, nsets, iters, rounds):
    lib = _lib.load()
    dh = H // nh
    gen = torch.Generator().manual_seed(42)
    w = lambda *s: (0.02 * torch.randn(*s, generator=gen)).to(DEV)
    w_order, b_order, w_dist, b_dist = w(2 * dh), w(1), w(2 * dh), w(1)
    scalar = torch.randn(1, generator=gen).to(DEV)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    sets = []
    for s in range(nsets):
        t = {k: rnd(B, L, H) for k in ("q", "k", "v", "qa", "ka", "d_cal", "d_att")}
        t["gate"] = torch.sigmoid(rnd(B, L, L))
        lens = torch.randint(1, L + 1, (B,), generator=gen)
        t["kv"] = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(DEV)

        def problem(adversarial):
            p = _lib.Problem()
            p.B, p.L, p.H, p.n_heads = B, L, H, nh
            p.q, p.k, p.v = _ptr(t["q"]), _ptr(t["k"]), _ptr(t["v"])
            p.mask_mode, p.causal, p.key_valid = _lib.MASK_STRUCTURED, 1, _ptr(t["kv"])
            p.w_order, p.b_order, p.w_dist, p.b_dist, p.scalar = (_ptr(x) for x in (w_order, b_order, w_dist, b_dist, scalar))
            p.adversarial, p.two_level = int(adversarial), 1
            p.rng_mode, p.p_drop, p.seed = _lib.RNG_COUNTER, 0.5, 1234 + s
            if adversarial:
                p.qa, p.ka, p.gate_logits, p.gate_is_prob = _ptr(t["qa"]), _ptr(t["ka"]), _ptr(t["gate"]), 1
                p.combine_option = _lib.COMBINE["gate"]
            return p

        ps, pa = problem(False), problem(True)
        t["affine"] = torch.zeros(B, nh, 4, 16 * ((L + 15) // 16), device=DEV)
        _lib.check(lib.acattn_spatial_affines(C.byref(ps), _ptr(t["affine"]), _stream()), "spatial_affines")
        ps_fwd = problem(False)
        ps_fwd.affine = _ptr(t["affine"])
        fo = _lib.FwdOut()
        t["ctx"] = torch.empty(B, L, H, device=DEV)
        fo.ctx_calibrated = _ptr(t["ctx"])
        # spatial-only backward
        sio = _lib.SpatialBwdIO()
        for k in ("dq", "dk", "dv"):
            t["s_" + k] = torch.empty(B, L, H, device=DEV)
        t["s_part"] = torch.empty(B * nh, 4 * dh + 4, device=DEV)
        t["s_ws"] = torch.empty(max(int(lib.acattn_spatial_attention_bwd_workspace_bytes(C.byref(ps))), 4) // 4, device=DEV)
        sio.d_ctx, sio.dq, sio.dk, sio.dv = _ptr(t["d_cal"]), _ptr(t["s_dq"]), _ptr(t["s_dk"]), _ptr(t["s_dv"])
        base = t["s_part"].data_ptr()
        sio.dw_order_part, sio.dw_dist_part, sio.dsmall_part, sio.part_stride = base, base + 8 * dh, base + 16 * dh, 4 * dh + 4
        sio.workspace = _ptr(t["s_ws"])
        # adversarial forward once (the backward reads its mask and row statistics), then its backward's buffers
        ao = _lib.FwdOut()
        t["a_ctx_att"], t["a_ctx_cal"] = torch.empty(B, L, H, device=DEV), torch.empty(B, L, H, device=DEV)
        t["M"] = torch.empty(B, nh, L, L, device=DEV)
        t["stats"] = torch.empty(B, nh, L, _lib.NSTAT, device=DEV)
        ao.ctx_attacked, ao.ctx_calibrated, ao.attack_mask, ao.row_stats = (_ptr(t[k]) for k in ("a_ctx_att", "a_ctx_cal", "M", "stats"))
        _lib.check(lib.acattn_calibrated_attention_fwd(C.byref(pa), C.byref(ao), _stream()), "adversarial fwd")
        aio = _lib.BwdIO()
        aio.attack_mask, aio.row_stats = _ptr(t["M"]), _ptr(t["stats"])
        aio.d_ctx_attacked, aio.d_ctx_calibrated = _ptr(t["d_att"]), _ptr(t["d_cal"])
        for k in ("dq", "dk", "dv", "dqa", "dka"):
            t["a_" + k] = torch.empty(B, L, H, device=DEV)
            setattr(aio, k, _ptr(t["a_" + k]))
        t["a_dgate"] = torch.empty(B, nh, L, L, device=DEV)
        aio.dgate_logits = _ptr(t["a_dgate"])
        t["a_part"] = torch.empty(B * nh, 4 * dh + 4, device=DEV)
        base = t["a_part"].data_ptr()
        aio.dw_order_part, aio.dw_dist_part, aio.dsmall_part, aio.part_stride = base, base + 8 * dh, base + 16 * dh, 4 * dh + 4
        t["a_ws"] = torch.empty(max(int(lib.acattn_calibrated_attention_bwd_workspace_bytes(C.byref(pa))), 4) // 4, device=DEV)
        aio.workspace = _ptr(t["a_ws"])
        sets.append((t, ps, ps_fwd, fo, sio, pa, aio))
    torch.cuda.synchronize()
    stream = _stream()

    def run(fn, *idx):
        def launch(i):
            s = sets[i]
            rc = fn(*(C.byref(s[j]) for j in idx), stream)
            if rc:
                _lib.check(rc, "launch")
        return _time(launch, nsets, iters, rounds)

    res = {"shape": {"B": B, "L": L, "H": H, "heads": nh, "p_drop": 0.5, "lengths": "U{1..L}", "mask": "structured causal"},
           "buffer_sets": nsets, "launches_per_round": iters, "rounds": rounds,
           "bytes_per_set_spatial_bwd": sum(sets[0][0][k].numel() * 4 for k in ("q", "k", "v", "d_cal", "s_dq", "s_dk", "s_dv"))}
    res["spatial_fwd"] = run(lib.acattn_calibrated_attention_fwd, 2, 3)
    res["spatial_bwd"] = run(lib.acattn_spatial_attention_bwd, 1, 4)
    lib.acattn_select_backward_kernel(_lib.BWD_STREAM)
    try:
        res["adversarial_bwd_stream"] = run(lib.acattn_calibrated_attention_bwd, 5, 6)
    finally:
        lib.acattn_select_backward_kernel(_lib.BWD_AUTO)
    res["adversarial_bwd_auto"] = run(lib.acattn_calibrated_attention_bwd, 5, 6)
    res["spatial_bwd_over_fwd"] = round(res["spatial_bwd"]["us"] / res["spatial_fwd"]["us"], 2)
    res["spatial_bwd_over_adversarial_stream"] = round(res["spatial_bwd"]["us"] / res["adversarial_bwd_stream"]["us"], 3)
    res["spatial_bwd_over_adversarial_auto"] = round(res["spatial_bwd"]["us"] / res["adversarial_bwd_auto"]["us"], 3)
    del sets
    torch.cuda.empty_cache()
    return res


def step_level(adversarial, B, L, items, warmup, steps, graph=True):
    torch.manual_seed(42)
    cfg = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, hidden_dropout_prob=0.5, attn_dropout_prob=0.5,
               hidden_act='gelu', layer_norm_eps=1e-12, initializer_range=0.02, loss_type='CE', combine_option='gate',
               two_level=True, use_order=True, use_distance=True, mask_loss_weight=0.03, use_position_embedding=True,
               MAX_ITEM_LIST_LENGTH=L, adversarial_calibrator=adversarial)
    model = A.ACSASRec(A.DictConfig(cfg), A.ItemCount(items)).to(DEV).train()
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-4), model)
    gen = torch.Generator().manual_seed(1000)
    pool = []
    for _ in range(8):
        lens = torch.randint(1, L + 1, (B,), generator=gen)
        ids = torch.randint(1, items, (B, L), generator=gen) * (torch.arange(L)[None] < lens[:, None])
        pool.append({"item_id_list": ids.to(DEV), "item_length": lens.to(DEV), "item_id": torch.randint(1, items, (B,), generator=gen).to(DEV)})
    if graph:
        trainer.enable_graph(pool[0])
    for i in range(warmup):
        trainer.train_step(pool[i % len(pool)])
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        last = trainer.train_step(pool[i % len(pool)])
        marks[i + 1].record()
    torch.cuda.synchronize()
    per = [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
    cal = float(last[1].detach())
    del trainer, model
    torch.cuda.empty_cache()
    return {"ms_per_step_median": round(statistics.median(per), 4), "ms_per_step_min": round(min(per), 4),
            "ms_per_step_max": round(max(per), 4), "steps": steps, "warmup": warmup, "final_calibrated_loss": round(cal, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nsets", type=int, default=6)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--census", action="store_true",
                    help="only the spatial-only training steps (for a rocprofv3 --kernel-trace run; tools/step_census.py reads the trace)")
    ap.add_argument("--no-graph", action="store_true", help="with --census: eager steps instead of hipGraph replays")
    a = ap.parse_args()
    if a.census:
        print(json.dumps({"census_run": step_level(False, 512, 50, a.items, a.warmup, a.steps, graph=not a.no_graph)}), flush=True)
        return
    assert a.iters >= 200 and a.nsets >= 5, "SURVEY 8d: >= 5 rotating buffer sets, >= 200 launches between events"
    out = {"tool": "tools/bench_spatial_only.py", "device": torch.cuda.get_device_name(0),
           "kernels": [kernel_level(512, 50, 64, 2, a.nsets, a.iters, a.rounds),
                       kernel_level(512, 200, 128, 4, max(5, a.nsets - 1), a.iters, a.rounds)]}
    if not a.skip_step:
        spatial = step_level(False, 512, 50, a.items, a.warmup, a.steps)
        full = step_level(True, 512, 50, a.items, a.warmup, a.steps)
        out["step"] = {"workload": f"ACSASRec 2 layers, {a.items} items, B=512 L=50 d=64 h=2, CE, Adam, hipGraph replay per step",
                       "spatial_only": spatial, "full_ac_sasrec": full,
                       "spatial_over_full": round(spatial["ms_per_step_median"] / full["ms_per_step_median"], 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
