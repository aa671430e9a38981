#!/usr/bin/env python3
"""Front-end timing for ACSSEPT's personalised front end (acattn_embed_user_layernorm_fwd / _bwd) beside the item-only front
end (acattn_embed_layernorm_fwd / _bwd) at the same rows and hidden size, on the GPU, through the C ABI.

Shape: B = 512, L = 50, 64 + 64 (H = 128), 12,102 items, 20,000 users, position table on, dropout 0.5 from the counter RNG.
Each sample is a device-event pair around `--inner` back-to-back launches of one kernel; the four kernels alternate inside every
round, so that drift of the shared machine hits them alike; the figure per kernel is the median over `--rounds` samples, with
the 10th / 90th percentiles beside it.  The new backward is timed in both designs of the user-table gradient (include/acattn.h:
user_rows_ws given = summed over each sequence's positions first, the default of the binding; NULL = scattered per row); the
sum-first figure covers both of its launches.  The backward accumulates into its gradient buffers without a zero fill in between
(the fill belongs to the caller and is the same for both).

The yardstick: the new kernel writes the same bytes, reads fewer table bytes and adds one index stream, so it should take no more
than 1.25 x the item-only kernel each way.  The verdict is printed, nothing is tuned to it.

`--core`: the un-normalised attention core of ACSSEPT (acattn_unnorm_attention_fwd / _bwd) beside the normalised core's
row-resident kernels (acattn_calibrated_attention_fwd pinned to ACATTN_FWD_STAGED, _bwd to ACATTN_BWD_ROW) in the same process,
at B = 512, L = 50, H = 128, 2 heads (head size 64), counter RNG, p_drop 0.5: forward, backward with all three cotangents,
and the attack-only backward (d_ctx_calibrated + d_penalty_part, attack_only = 1).  Same sampling as above.  No bar is set.

Usage:  python tools/bench_ssept.py [--core] [--out profiles/ssept_front_end.txt | profiles/ssept_core.txt]
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ac_tsr_amd import _lib  # noqa: E402
from ac_tsr_amd.ops import _ptr, _stream  # noqa: E402


def sample(kernels, a):
    """{name: [us per launch, ...]}: `a.rounds` device-event samples of `a.inner` launches each, the kernels alternating."""
    for _ in range(a.warmup):
        for fn in kernels.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in kernels}
    for _ in range(a.rounds):
        for k, fn in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            samples[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    return samples


def core(a):
    from ac_tsr_amd import attn_launch
    dev, lib = "cuda", _lib.load()
    B, L, H, nh, p_drop = 512, 50, 128, 2, 0.5
    dh, nqb = H // nh, (L + 15) // 16
    g = torch.Generator().manual_seed(0)
    f = lambda *s: torch.randn(*s, generator=g).to(dev)
    q, k, v, qa, ka, gl = f(B, L, H), f(B, L, H), f(B, L, H), f(B, L, H), f(B, L, H), f(B, L, L)
    scale = 0.3 * (32 / dh) ** 0.5
    w_order, b_order, w_dist, b_dist, scalar = scale * f(2 * dh), scale * f(1), scale * f(2 * dh), scale * f(1), scale * f(1)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    kv = (torch.arange(L)[None, :] < lens[:, None]).to(torch.uint8).to(dev)
    prob = attn_launch.fill_problem(q, k, v, qa, ka, gl, w_order, b_order, w_dist, b_dist, scalar, nh, p_drop, 1234, None,
                                    key_valid=kv, causal=True)
    e = lambda *s: torch.empty(*s, device=dev)
    outs = {}
    for name in ("unnorm", "norm"):
        o = _lib.FwdOut()
        t = dict(ctx_a=e(B, L, H), ctx_c=e(B, L, H), M=e(B, nh, L, L), stats=e(B, nh, L, _lib.NSTAT))
        o.ctx_attacked, o.ctx_calibrated, o.attack_mask, o.row_stats = _ptr(t["ctx_a"]), _ptr(t["ctx_c"]), _ptr(t["M"]), _ptr(t["stats"])
        outs[name] = (o, t)
    d_att, d_cal, d_M, d_pen = f(B, L, H), f(B, L, H), 1e-3 * f(B, nh, L, L), 1e-3 * f(B, nh, nqb)
    ws = attn_launch.workspace(lib.acattn_calibrated_attention_bwd_workspace_bytes(C.byref(prob)), dev)
    ios = {}
    for name in ("unnorm", "norm"):
        for pattern in ("all", "attack"):
            io = _lib.BwdIO()
            t = dict(g=[e(B, L, H) for _ in range(5)], gate=e(B, nh, L, L), part=e(B * nh, 4 * dh + 4))
            io.attack_mask, io.row_stats = _ptr(outs[name][1]["M"]), _ptr(outs[name][1]["stats"])
            if pattern == "all":
                io.d_ctx_attacked, io.d_ctx_calibrated, io.d_attack_mask = _ptr(d_att), _ptr(d_cal), _ptr(d_M)
            else:
                io.d_ctx_calibrated, io.d_penalty_part, io.attack_only = _ptr(d_cal), _ptr(d_pen), 1
            io.dq, io.dk, io.dv, io.dqa, io.dka = (_ptr(x) for x in t["g"])
            io.dgate_logits = _ptr(t["gate"])
            base = t["part"].data_ptr()
            io.dw_order_part, io.dw_dist_part, io.dsmall_part, io.part_stride = base, base + 8 * dh, base + 16 * dh, 4 * dh + 4
            if name == "norm":
                io.workspace = _ptr(ws)
            ios[name, pattern] = (io, t)
    lib.acattn_select_forward_kernel(_lib.FWD_STAGED)
    lib.acattn_select_backward_kernel(_lib.BWD_ROW)
    chk = lambda rc: _lib.check(rc, "core")
    kernels = {
        "unnorm fwd": lambda: chk(lib.acattn_unnorm_attention_fwd(C.byref(prob), C.byref(outs["unnorm"][0]), _stream())),
        "norm   fwd": lambda: chk(lib.acattn_calibrated_attention_fwd(C.byref(prob), C.byref(outs["norm"][0]), _stream())),
        "unnorm bwd all": lambda: chk(lib.acattn_unnorm_attention_bwd(C.byref(prob), C.byref(ios["unnorm", "all"][0]), _stream())),
        "norm   bwd all": lambda: chk(lib.acattn_calibrated_attention_bwd(C.byref(prob), C.byref(ios["norm", "all"][0]), _stream())),
        "unnorm bwd attack": lambda: chk(lib.acattn_unnorm_attention_bwd(C.byref(prob), C.byref(ios["unnorm", "attack"][0]), _stream())),
        "norm   bwd attack": lambda: chk(lib.acattn_calibrated_attention_bwd(C.byref(prob), C.byref(ios["norm", "attack"][0]), _stream())),
    }
    samples = sample(kernels, a)
    lib.acattn_select_forward_kernel(_lib.FWD_AUTO)
    lib.acattn_select_backward_kernel(_lib.BWD_AUTO)
    assert all(torch.isfinite(t).all() for t in outs["unnorm"][1].values())
    assert all(torch.isfinite(t).all() for t in ios["unnorm", "all"][1]["g"])
    qt = lambda v, f_: sorted(v)[min(len(v) - 1, int(f_ * len(v)))]
    lines = [f"un-normalised attention core (acattn_unnorm.hip) vs the normalised row-resident kernels, B={B} L={L} H={H} heads={nh} "
             f"(head size {dh}), counter RNG, p_drop={p_drop}",
             f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds x {a.inner} launches per sample, kernels alternating; us per launch",
             "norm fwd: ACATTN_FWD_STAGED; norm bwd: ACATTN_BWD_ROW; `attack`: d_ctx_calibrated + d_penalty_part, attack_only = 1",
             f"{'kernel':<18} {'median':>8} {'p10':>8} {'p90':>8}"]
    for name, vals in samples.items():
        lines.append(f"{name:<18} {qt(vals, 0.5):8.2f} {qt(vals, 0.1):8.2f} {qt(vals, 0.9):8.2f}")
    for way in ("fwd", "bwd all", "bwd attack"):
        r = qt(samples[f"unnorm {way}"], 0.5) / qt(samples[f"norm   {way}"], 0.5)
        lines.append(f"{way}: unnorm / norm = {r:.3f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--core", action="store_true", help="time the un-normalised attention core beside the normalised one")
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ssept.py measures on the GPU; there is no CPU path"
    if a.core:
        return core(a)
    dev = "cuda"
    lib = _lib.load()
    B, L, Di, Du, N, U, p_drop = 512, 50, 64, 64, 12102, 20000, 0.5
    H, rows, chunks = Di + Du, B * L, _lib.EMBED_BWD_CHUNKS
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    idx = (torch.randint(1, N, (B, L), generator=g) * (torch.arange(L)[None, :] < lens[:, None])).to(dev)
    uid = torch.randint(1, U, (B,), generator=g).to(dev)
    f = lambda *s: torch.randn(*s, generator=g).to(dev)
    item, user, wide, pos, gamma, beta, dy = f(N, Di), f(U, Du), f(N, H), f(L, H), f(H), f(H), f(B, L, H)
    y, stats = torch.empty(B, L, H, device=dev), torch.empty(rows, 2, device=dev)
    nonzero = torch.empty(B, L, dtype=torch.uint8, device=dev)
    d_item, d_user, d_wide = torch.zeros_like(item), torch.zeros_like(user), torch.zeros_like(wide)
    pos_part, gb_part = torch.empty(chunks, L, H, device=dev), torch.empty(chunks * L, 2, H, device=dev)
    user_rows = torch.empty(rows, Du, device=dev)

    pu = _lib.EmbedUserProblem()
    pu.rows, pu.L, pu.H, pu.Di, pu.n_table_rows, pu.n_user_rows = rows, L, H, Di, N, U
    pu.idx, pu.user, pu.table, pu.user_table = _ptr(idx), _ptr(uid), _ptr(item), _ptr(user)
    pe = _lib.EmbedProblem()
    pe.rows, pe.L, pe.H, pe.n_table_rows = rows, L, H, N
    pe.idx, pe.table = _ptr(idx), _ptr(wide)
    for p in (pu, pe):
        p.pos, p.gamma, p.beta, p.eps, p.p_drop, p.seed, p.nonzero_out = _ptr(pos), _ptr(gamma), _ptr(beta), 1e-12, p_drop, 1234, _ptr(nonzero)

    def call(rc, what):
        _lib.check(rc, what)

    # each backward needs the (mean, 1/std) of ITS forward: one stats buffer per front end
    stats_u, stats_e = torch.empty_like(stats), torch.empty_like(stats)
    kernels = {
        "embed_user fwd": lambda: call(lib.acattn_embed_user_layernorm_fwd(C.byref(pu), _ptr(y), _ptr(stats_u), _stream()), "fwd"),
        "embed      fwd": lambda: call(lib.acattn_embed_layernorm_fwd(C.byref(pe), _ptr(y), _ptr(stats_e), _stream()), "fwd"),
        # the two designs of the user-table gradient: a row sum over each sequence's positions first / one atomic per row
        "embed_user bwd": lambda: call(lib.acattn_embed_user_layernorm_bwd(
            C.byref(pu), _ptr(dy), _ptr(stats_u), 0, 0, _ptr(d_item), _ptr(d_user), _ptr(user_rows), _ptr(pos_part), _ptr(gb_part),
            _stream()), "bwd"),
        "  (scatter) bwd": lambda: call(lib.acattn_embed_user_layernorm_bwd(
            C.byref(pu), _ptr(dy), _ptr(stats_u), 0, 0, _ptr(d_item), _ptr(d_user), None, _ptr(pos_part), _ptr(gb_part),
            _stream()), "bwd"),
        "embed      bwd": lambda: call(lib.acattn_embed_layernorm_bwd(
            C.byref(pe), _ptr(dy), _ptr(stats_e), 0, _ptr(d_wide), _ptr(pos_part), _ptr(gb_part), _stream()), "bwd"),
    }
    for _ in range(a.warmup):
        for fn in kernels.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in kernels}
    for _ in range(a.rounds):
        for k, fn in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            samples[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)  # us per launch
    assert all(torch.isfinite(t).all() for t in (y, d_item, d_user, d_wide))
    q = lambda v, f_: sorted(v)[min(len(v) - 1, int(f_ * len(v)))]
    med = {k: q(v, 0.5) for k, v in samples.items()}
    n_pad = int((idx == 0).sum())
    lines = [f"ACSSEPT front end vs item-only front end, B={B} L={L} H={H} (item {Di} + user {Du}), {N} items, {U} users, "
             f"pos on, p_drop={p_drop} (counter RNG); {n_pad} of {rows} lookups are padding",
             f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds x {a.inner} launches per sample, kernels alternating; us per launch",
             f"{'kernel':<16} {'median':>8} {'p10':>8} {'p90':>8}"]
    for k, v in samples.items():
        lines.append(f"{k:<16} {med[k]:8.2f} {q(v, 0.1):8.2f} {q(v, 0.9):8.2f}")
    # bytes the algorithm moves (gathers counted per lookup; what hits in cache is the hardware's business)
    out_b = rows * H * 4 + rows * 8 + rows
    fwd_u = rows * Di * 4 + rows * Du * 4 + rows * 8 + B * 8 + out_b
    fwd_e = rows * H * 4 + rows * 8 + out_b
    lines.append(f"forward bytes per launch (every lookup counted): embed_user {fwd_u}, embed {fwd_e}; distinct user-row bytes {B * Du * 4}")
    for way in ("fwd", "bwd"):
        r = med[f"embed_user {way}"] / med[f"embed      {way}"]
        lines.append(f"{way}: embed_user / embed = {r:.3f}  ->  {'within' if r <= 1.25 else 'OVER'} the 1.25 x yardstick")
    r = med["  (scatter) bwd"] / med["embed      bwd"]
    lines.append(f"bwd, user rows scattered per (b, l) instead of summed first: {r:.3f} x embed")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
