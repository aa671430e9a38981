#!/usr/bin/env python3
"""bench_long_sequences.py: what the long form of the attention core (208 < L <= 496) costs on the MI355X.

(a) kernel level, B = 512, H = 64, 2 heads, structured causal mask, counter RNG, p_drop 0.5, gate combine, item_length ~
    U{1..L}; forward (acattn_calibrated_attention_fwd, penalty sums included) and backward (acattn_calibrated_attention_bwd,
    both context cotangents, dense) launch times:
      L = 208  today's streaming kernels (automatic choice)
      L = 208  the long form pinned (ACATTN_FWD_LONG / ACATTN_BWD_LONG): the price of recomputing the products per sweep
      L = 256  the long form (automatic choice)
      L = 496  the long form (automatic choice)
    each over >= 5 rotating buffer sets (working set beyond the 256 MB Infinity Cache), `--iters` launches between two
    device events (`--iters-long` above 208 keys: those launches take milliseconds), median of the rounds;
(b) step level: the eager train_step of a 2-layer ACSASRec (two-pass protocol, Adam) at L = 256, B = 128, 20k items, medians
    of per-step device-event times.

Prints ONE JSON line.  Measurement helper, not product; needs the GPU; reads nothing outside the repository."""
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
    for i in range(min(10, iters)):
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
    return {"us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}


def kernel_level(L, pin_long, nsets, iters, rounds, B=512, H=64, nh=2):
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
        t["gate"] = rnd(B, L, L)
        lens = torch.randint(1, L + 1, (B,), generator=gen)
        t["kv"] = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(DEV)
        p = _lib.Problem()
        p.B, p.L, p.H, p.n_heads = B, L, H, nh
        p.q, p.k, p.v, p.qa, p.ka, p.gate_logits = (_ptr(t[k]) for k in ("q", "k", "v", "qa", "ka", "gate"))
        p.mask_mode, p.causal, p.key_valid = _lib.MASK_STRUCTURED, 1, _ptr(t["kv"])
        p.w_order, p.b_order, p.w_dist, p.b_dist, p.scalar = (_ptr(x) for x in (w_order, b_order, w_dist, b_dist, scalar))
        p.adversarial, p.two_level, p.combine_option = 1, 1, _lib.COMBINE["gate"]
        p.rng_mode, p.p_drop, p.seed = _lib.RNG_COUNTER, 0.5, 1234 + s
        fo = _lib.FwdOut()
        t["ctx_att"], t["ctx_cal"] = torch.empty(B, L, H, device=DEV), torch.empty(B, L, H, device=DEV)
        t["M"] = torch.empty(B, nh, L, L, device=DEV)
        t["stats"] = torch.empty(B, nh, L, _lib.NSTAT, device=DEV)
        t["pen"] = torch.empty(B, nh, (L + 15) // 16, device=DEV)
        fo.ctx_attacked, fo.ctx_calibrated, fo.attack_mask, fo.row_stats, fo.penalty_part = (
            _ptr(t[k]) for k in ("ctx_att", "ctx_cal", "M", "stats", "pen"))
        io = _lib.BwdIO()
        io.attack_mask, io.row_stats = _ptr(t["M"]), _ptr(t["stats"])
        io.d_ctx_attacked, io.d_ctx_calibrated = _ptr(t["d_att"]), _ptr(t["d_cal"])
        for k in ("dq", "dk", "dv", "dqa", "dka"):
            t["g_" + k] = torch.empty(B, L, H, device=DEV)
            setattr(io, k, _ptr(t["g_" + k]))
        t["dgate"] = torch.empty(B, nh, L, L, device=DEV)
        io.dgate_logits = _ptr(t["dgate"])
        t["part"] = torch.empty(B * nh, 4 * dh + 4, device=DEV)
        base = t["part"].data_ptr()
        io.dw_order_part, io.dw_dist_part, io.dsmall_part, io.part_stride = base, base + 8 * dh, base + 16 * dh, 4 * dh + 4
        t["ws"] = torch.empty(max(int(lib.acattn_calibrated_attention_bwd_workspace_bytes(C.byref(p))), 4) // 4, device=DEV)
        io.workspace = _ptr(t["ws"])
        sets.append((t, p, fo, io))
    torch.cuda.synchronize()
    stream = _stream()

    def run(fn, a, b):
        def launch(i):
            s = sets[i]
            rc = fn(C.byref(s[a]), C.byref(s[b]), stream)
            if rc:
                _lib.check(rc, "launch")
        return _time(launch, nsets, iters, rounds)

    lib.acattn_select_forward_kernel(_lib.FWD_LONG if pin_long else _lib.FWD_AUTO)
    lib.acattn_select_backward_kernel(_lib.BWD_LONG if pin_long else _lib.BWD_AUTO)
    try:
        fwd = run(lib.acattn_calibrated_attention_fwd, 1, 2)  # (also leaves every set's M and row_stats for the backward)
        bwd = run(lib.acattn_calibrated_attention_bwd, 1, 3)
    finally:
        lib.acattn_select_forward_kernel(_lib.FWD_AUTO)
        lib.acattn_select_backward_kernel(_lib.BWD_AUTO)
    finite = all(bool(torch.isfinite(s[0]["g_dq"]).all()) and bool(torch.isfinite(s[0]["ctx_cal"]).all()) for s in sets)
    res = {"L": L, "form": "long" if (pin_long or L > 208) else "streaming", "pinned": bool(pin_long), "B": B, "H": H, "heads": nh,
           "buffer_sets": nsets, "launches_per_round": iters, "rounds": rounds, "fwd": fwd, "bwd": bwd,
           "fwd_plus_bwd_us": round(fwd["us"] + bwd["us"], 1), "outputs_finite": finite}
    del sets
    torch.cuda.empty_cache()
    return res


def step_level(L, B, items, warmup, steps):
    torch.manual_seed(42)
    cfg = dict(n_layers=2, n_heads=2, hidden_size=64, inner_size=256, hidden_dropout_prob=0.5, attn_dropout_prob=0.5,
               hidden_act='gelu', layer_norm_eps=1e-12, initializer_range=0.02, loss_type='CE', combine_option='gate',
               two_level=True, use_order=True, use_distance=True, mask_loss_weight=0.03, MAX_ITEM_LIST_LENGTH=L, gate_seq_length=L)
    model = A.ACSASRec(A.DictConfig(cfg), A.ItemCount(items)).to(DEV).train()
    trainer = A.AttackSASRecTrainer(A.DictConfig(learner='adam', learning_rate=1e-4), model)
    gen = torch.Generator().manual_seed(1000)
    pool = []
    for _ in range(4):
        lens = torch.randint(1, L + 1, (B,), generator=gen)
        ids = torch.randint(1, items, (B, L), generator=gen) * (torch.arange(L)[None] < lens[:, None])
        pool.append({"item_id_list": ids.to(DEV), "item_length": lens.to(DEV), "item_id": torch.randint(1, items, (B,), generator=gen).to(DEV)})
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
    return {"workload": f"ACSASRec 2 layers, {items} items, B={B} L={L} d=64 h=2, CE, Adam, two-pass protocol, eager steps",
            "ms_per_step_median": round(statistics.median(per), 3), "ms_per_step_min": round(min(per), 3),
            "ms_per_step_max": round(max(per), 3), "steps": steps, "warmup": warmup,
            "final_losses": [round(float(x.detach()), 4) for x in last]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--iters-long", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nsets", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    assert a.nsets >= 5, ">= 5 rotating buffer sets"
    rows = [kernel_level(208, False, a.nsets, a.iters, a.rounds), kernel_level(208, True, a.nsets, a.iters_long, a.rounds),
            kernel_level(256, False, a.nsets, a.iters_long, a.rounds), kernel_level(496, False, a.nsets, a.iters_long, a.rounds)]
    out = {"tool": "tools/bench_long_sequences.py", "device": torch.cuda.get_device_name(0), "kernels": rows,
           "long_over_streaming_at_208": {"fwd": round(rows[1]["fwd"]["us"] / rows[0]["fwd"]["us"], 2),
                                          "bwd": round(rows[1]["bwd"]["us"] / rows[0]["bwd"]["us"], 2)}}
    if not a.skip_step:
        out["step"] = step_level(256, 128, 20_000, a.warmup, a.steps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
