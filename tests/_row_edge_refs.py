"""Inputs and fp64 torch references of the row-edge tests (tests/test_hip_row_edges_*.py), CPU only.

Each `*_case` builds the fp32 inputs of one launch from a seeded generator; each `*_ref` evaluates the operation the header
(include/acattn.h) describes with torch ops in fp64 and returns every tensor the launch writes, by the name of its pointer.
tests/test_guarded_cpu.py evaluates each reference at the smallest shape of its family and asserts that it is finite wherever
the GPU tests demand "no poison", so that demand is one the reference alone meets.
"""
from __future__ import annotations

import torch

LN_BWD_GRID = 512        # ACATTN_LN_BWD_GRID
EMBED_BWD_CHUNKS = 8     # ACATTN_EMBED_BWD_CHUNKS
FWD_GRID_CAP = 2048      # launch_fwd of acattn_ln.hip / acattn_embed.hip / acattn_embed_user.hip


def rpb(H: int) -> int:
    """Rows per workgroup pass of the row kernels: 256 threads, H / 4 lanes per row."""
    return 256 // (H // 4)


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(sum(int(k) * m for k, m in zip(key, (1, 7919, 104729, 1299709, 15485863))))


# ---------------------------------------------------------------------------------------------------------------------------
# y = LayerNorm(dropout(z) + residual)
def ln_case(H, rows, residual_rows, p):
    g = _gen(H, rows, residual_rows, int(p * 10))
    c = {"H": H, "rows": rows, "residual_rows": residual_rows, "p": p}
    c["z"] = torch.randn(rows, H, generator=g)
    c["residual"] = torch.randn(residual_rows, H, generator=g)
    c["gamma"] = 1 + 0.3 * torch.randn(H, generator=g)
    c["beta"] = 0.3 * torch.randn(H, generator=g)
    c["keep"] = torch.empty(rows, H).bernoulli_(1 - p, generator=g).to(torch.uint8) if p > 0 else None
    c["dy"] = torch.randn(rows, H, generator=g)
    return c


def ln_ref(c, eps=1e-12):
    """y, stats of acattn_dropout_add_layernorm_fwd; dz, dres (per row, not folded over a broadcast residual), dgamma, dbeta
    of _bwd (the kernel's dgb_part [512, 2, H] must SUM to the last two)."""
    H, rows, rr, p = c["H"], c["rows"], c["residual_rows"], c["p"]
    scale = c["keep"].double() / (1 - p) if c["keep"] is not None else torch.ones(rows, H, dtype=torch.float64)
    res = c["residual"].double()[torch.arange(rows) % rr]
    s = (c["z"].double() * scale + res).requires_grad_(True)
    gm, bt = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(s, (H,), gm, bt, eps)
    ds, dgamma, dbeta = torch.autograd.grad((y * c["dy"].double()).sum(), [s, gm, bt])
    sd = s.detach()
    mean = sd.mean(-1)
    rstd = (sd.var(-1, unbiased=False) + eps).rsqrt()
    return {"y": y.detach(), "stats": torch.stack([mean, rstd], -1), "dz": ds * scale, "dres": ds, "dgamma": dgamma,
            "dbeta": dbeta}


def ln_rows(H):
    """Row counts of the LayerNorm cases.  Forward: one pass of min(ceil(rows / RPB), 2048) workgroups of RPB rows; the
    grid-stride loop makes a second pass above 2048 * RPB rows.  Backward: always 512 workgroups (ACATTN_LN_BWD_GRID), so
    workgroups without rows exist below 512 * RPB rows and a second pass above."""
    r = rpb(H)
    return [1, r - 1, r, r + 1, LN_BWD_GRID * r - 1, LN_BWD_GRID * r + 1, FWD_GRID_CAP * r - 1, FWD_GRID_CAP * r,
            FWD_GRID_CAP * r + 1, 2 * FWD_GRID_CAP * r + 3]


# ---------------------------------------------------------------------------------------------------------------------------
# y = dropout(LayerNorm(table[idx] + pos))
def embed_case(H, B, L, N, p, with_pos=True, bad_ids=True):
    g = _gen(H, B, L, N, int(p * 10))
    c = {"H": H, "B": B, "L": L, "N": N, "p": p}
    idx = torch.randint(0, N, (B, L), generator=g)
    flat = idx.view(-1)
    flat[-1] = N - 1                       # the last table row is hit (its gradient row ends at d_table's back guard)
    if bad_ids and flat.numel() >= 4:      # ids outside [0, N) are clamped (header: "never dereferenced out of bounds")
        flat[0], flat[1] = -1, N
    if flat.numel() >= 3:
        flat[2] = 0                        # a padding id
    c["idx"] = idx
    c["table"] = torch.randn(N, H, generator=g)
    c["pos"] = 0.5 * torch.randn(L + 3, H, generator=g) if with_pos else None
    c["gamma"] = 1 + 0.3 * torch.randn(H, generator=g)
    c["beta"] = 0.3 * torch.randn(H, generator=g)
    c["keep"] = torch.empty(B * L, H).bernoulli_(1 - p, generator=g).to(torch.uint8) if p > 0 else None
    c["dy"] = torch.randn(B * L, H, generator=g)
    return c


def _norm_with_grads(x, gamma, beta, scale, dy, eps):
    """LayerNorm(x) * scale with cotangent dy: (y, stats, d x, dgamma, dbeta), all fp64."""
    H = x.shape[-1]
    x = x.detach().requires_grad_(True)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (H,), gm, bt, eps) * scale
    dx, dgamma, dbeta = torch.autograd.grad((y * dy.double()).sum(), [x, gm, bt])
    xd = x.detach()
    stats = torch.stack([xd.mean(-1), (xd.var(-1, unbiased=False) + eps).rsqrt()], -1)
    return y.detach(), stats, dx, dgamma, dbeta


def embed_ref(c, padding_idx=0, eps=1e-12):
    """y [rows,H], stats [rows,2], nonzero [rows] of acattn_embed_layernorm_fwd; d_table [N,H] (rows of the CLAMPED id ==
    padding_idx skipped), d_pos [L,H], dgamma, dbeta [H] of _bwd (the partial buffers must SUM to the last three)."""
    H, B, L, N, p = c["H"], c["B"], c["L"], c["N"], c["p"]
    rows = B * L
    raw = c["idx"].reshape(-1)
    ids = raw.clamp(0, N - 1)
    scale = c["keep"].double() / (1 - p) if c["keep"] is not None else torch.ones(rows, H, dtype=torch.float64)
    x = c["table"].double()[ids]
    if c["pos"] is not None:
        x = x + c["pos"].double()[torch.arange(rows) % L]
    y, stats, dx, dgamma, dbeta = _norm_with_grads(x, c["gamma"], c["beta"], scale, c["dy"], eps)
    d_table = torch.zeros(N, H, dtype=torch.float64)
    live = ids != padding_idx
    d_table.index_add_(0, ids[live], dx[live])
    d_pos = dx.view(B, L, H).sum(0)
    return {"y": y, "stats": stats, "nonzero": (raw != 0).to(torch.uint8), "d_table": d_table, "d_pos": d_pos,
            "dgamma": dgamma, "dbeta": dbeta}


def embed_shapes(H):
    """(B, L) of the embedding cases: rows = B * L around 1, RPB, the forward's single-pass limit 2048 * RPB, and into its
    second pass; L = 50 crosses the limit inside a sequence.  The backward runs L x 8 workgroups, each over ceil(B / 8)
    sequences at one position: B < 8 leaves workgroups without rows."""
    r = rpb(H)
    cap = FWD_GRID_CAP * r
    return [(1, 1), (r - 1, 1), (r, 1), (r + 1, 1), (1, 50), (cap - 1, 1), (cap, 1), (cap + 1, 1), (cap // 50 + 1, 50),
            (2 * cap + 3, 1)]


# ---------------------------------------------------------------------------------------------------------------------------
# y = dropout(LayerNorm(cat(table[idx], user_table[user]) + pos))
def embed_user_case(H, Di, B, L, N, U, p, with_pos=True):
    g = _gen(H + Di, B, L, N + U, int(p * 10))
    c = embed_case(H, B, L, N, p, with_pos)
    c["table"] = torch.randn(N, Di, generator=g)
    c["Di"], c["U"] = Di, U
    user = torch.randint(0, U, (B,), generator=g)
    user[-1] = U - 1                       # the last user row is hit
    if B >= 4:
        user[0], user[1], user[2] = -1, U, 0  # clamped ids and the padding user
    if B >= 6:
        user[3] = user[4] = U - 1          # one user in several sequences
    c["user"] = user
    c["user_table"] = torch.randn(U, H - Di, generator=g)
    return c


def embed_user_ref(c, item_padding_idx=0, user_padding_idx=0, eps=1e-12):
    """As embed_ref, with d_item [N,Di], d_user [U,H-Di] and user_rows [rows,H-Di] (the user half of every row's gradient)."""
    H, Di, B, L, N, U, p = c["H"], c["Di"], c["B"], c["L"], c["N"], c["U"], c["p"]
    rows = B * L
    raw = c["idx"].reshape(-1)
    ids = raw.clamp(0, N - 1)
    uids = c["user"].clamp(0, U - 1)
    urow = uids.repeat_interleave(L)
    scale = c["keep"].double() / (1 - p) if c["keep"] is not None else torch.ones(rows, H, dtype=torch.float64)
    x = torch.cat([c["table"].double()[ids], c["user_table"].double()[urow]], -1)
    if c["pos"] is not None:
        x = x + c["pos"].double()[torch.arange(rows) % L]
    y, stats, dx, dgamma, dbeta = _norm_with_grads(x, c["gamma"], c["beta"], scale, c["dy"], eps)
    d_item = torch.zeros(N, Di, dtype=torch.float64)
    live = ids != item_padding_idx
    d_item.index_add_(0, ids[live], dx[live, :Di])
    d_user = torch.zeros(U, H - Di, dtype=torch.float64)
    live = urow != user_padding_idx
    d_user.index_add_(0, urow[live], dx[live, Di:])
    return {"y": y, "stats": stats, "nonzero": (raw != 0).to(torch.uint8), "d_item": d_item, "d_user": d_user,
            "user_rows": dx[:, Di:].contiguous(), "d_pos": dx.view(B, L, H).sum(0), "dgamma": dgamma, "dbeta": dbeta}


# ---------------------------------------------------------------------------------------------------------------------------
# the small reductions and loss finishers of acattn_util.hip
def sum_rows_ref(x):
    """out[bt, c] = sum_r x[bt, r, c]."""
    return x.double().sum(1)


def dense_ce_case(rows, N):
    g = _gen(rows, N, 3)
    c = {"rows": rows, "N": N, "logits": 3 * torch.randn(rows, N, generator=g), "coef": torch.randn(rows, generator=g)}
    c["target"] = torch.randint(0, N, (rows,), generator=g)
    c["target"][-1] = N - 1                # the last column is a target
    return c


def dense_ce_ref(c):
    """lse, row_loss of acattn_dense_ce_fwd; d_logits of _bwd."""
    lg = c["logits"].double()
    lse = torch.logsumexp(lg, -1)
    row_loss = lse - lg.gather(1, c["target"][:, None])[:, 0]
    onehot = torch.zeros_like(lg).scatter_(1, c["target"][:, None], 1.0)
    d_logits = c["coef"].double()[:, None] * (torch.exp(lg - lse[:, None]) - onehot)
    return {"lse": lse, "row_loss": row_loss, "d_logits": d_logits}


def penalty_rows_ref(m):
    """pen[b, head, qb] = sum over the 16 rows of query block qb and all L keys of (1 - M)^2; M [B,nh,L,L]."""
    B, nh, L, _ = m.shape
    nqb = (L + 15) // 16
    per_row = ((1 - m.double()) ** 2).sum(-1)
    pad = torch.zeros(B, nh, nqb * 16, dtype=torch.float64)
    pad[:, :, :L] = per_row
    return pad.view(B, nh, nqb, 16).sum(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# the layer tail: a = LayerNorm(dropout(dense(ctx)) + x); out = LayerNorm(dropout(dense_2(gelu(dense_1(a)))) + a)
TAIL_PARAMS = ("wd", "bd", "g1", "b1", "w1", "bb1", "w2", "bb2", "g2", "b2")


def tail_case(H, I, rows, p, pick=False):
    """Inputs of one tail launch (the weights scaled as in tests/test_hip_tail.py: products stay O(1) at every width).
    `pick`: a row selection -- ctx, x are [B, 5, H], the tail runs on rows = B * R positions src_index of them, R = 3 when 3
    divides rows (then the first two picks of every sequence are the same position), else 1; positions -1 and 5 occur (the
    kernel clamps them, include/acattn.h: acattn_bwd_io.read_rows states the same precondition)."""
    g = _gen(H, I, rows, int(p * 10), int(pick))
    r = lambda *s: torch.randn(*s, generator=g)
    scale = 0.3 * (64 / H) ** 0.5
    c = {"H": H, "I": I, "rows": rows, "p": p, "src_index": None, "src_R": 0, "src_L": 0}
    src_rows = rows
    if pick:
        R = 3 if rows % 3 == 0 else 1
        B, L = rows // R, 5
        pos = torch.randint(-1, L + 1, (B, R), generator=g)
        pos.view(-1)[0], pos.view(-1)[-1] = -1, L
        if R == 3:
            pos[:, 1] = pos[:, 0]
        c["src_index"], c["src_R"], c["src_L"] = pos.reshape(-1), R, L
        src_rows = B * L
    c["src_rows"] = src_rows
    c.update(ctx=r(src_rows, H), x=r(src_rows, H), wd=scale * r(H, H), bd=0.1 * r(H), g1=1 + 0.3 * r(H), b1=0.3 * r(H),
             w1=scale * r(I, H), bb1=0.1 * r(I), w2=scale * r(H, I), bb2=0.1 * r(H), g2=1 + 0.3 * r(H), b2=0.3 * r(H))
    for k in ("keep1", "keep2"):
        c[k] = torch.empty(rows, H).bernoulli_(1 - p, generator=g).to(torch.uint8) if p > 0 else None
    c["d_out"] = r(rows, H)
    return c


def tail_source_rows(c):
    """Row of ctx / x each tail row reads (include/acattn.h: (r / src_R) * src_L + src_index[r], positions clamped)."""
    rows = c["rows"]
    if c["src_index"] is None:
        return torch.arange(rows)
    return (torch.arange(rows) // c["src_R"]) * c["src_L"] + c["src_index"].clamp(0, c["src_L"] - 1)


def tail_ref(c, eps=1e-12):
    """Everything acattn_layer_tail_fwd writes (h1, st1, a, act, h3, st2, out, gelu_grad) and acattn_layer_tail_bwd writes
    (d_ctx, d_x over the SOURCE rows -- added where a position is picked twice --, d_h1, d_h2, d_h3, and dgb [4, H] =
    (dgamma1, dbeta1, dgamma2, dbeta2), which the kernel's dgb_part must sum to), fp64."""
    F = torch.nn.functional
    H, p = c["H"], c["p"]
    d = {k: c[k].double() for k in TAIL_PARAMS}
    for k in ("g1", "b1", "g2", "b2"):
        d[k].requires_grad_(True)
    src = tail_source_rows(c)
    cx = c["ctx"].double()[src].requires_grad_(True)
    xx = c["x"].double()[src].requires_grad_(True)
    drop = lambda z, k: z if k is None else z * (k.double() / (1 - p))
    h1 = F.linear(cx, d["wd"], d["bd"])
    s1 = drop(h1, c["keep1"]) + xx
    a = F.layer_norm(s1, (H,), d["g1"], d["b1"], eps)
    h2 = F.linear(a, d["w1"], d["bb1"])
    act = F.gelu(h2)
    h3 = F.linear(act, d["w2"], d["bb2"])
    s2 = drop(h3, c["keep2"]) + a
    out = F.layer_norm(s2, (H,), d["g2"], d["b2"], eps)
    g = torch.autograd.grad((out * c["d_out"].double()).sum(), [cx, xx, h1, h2, h3, d["g1"], d["b1"], d["g2"], d["b2"]])
    stats = lambda s: torch.stack([s.mean(-1), (s.var(-1, unbiased=False) + eps).rsqrt()], -1).detach()
    h2d = h2.detach()
    gelu_grad = 0.5 * (1 + torch.erf(h2d / 2 ** 0.5)) + h2d * torch.exp(-0.5 * h2d * h2d) / (2 * torch.pi) ** 0.5
    d_ctx = torch.zeros(c["src_rows"], H, dtype=torch.float64).index_add_(0, src, g[0])
    d_x = torch.zeros(c["src_rows"], H, dtype=torch.float64).index_add_(0, src, g[1])
    return {"h1": h1.detach(), "st1": stats(s1), "a": a.detach(), "act": act.detach(), "h3": h3.detach(), "st2": stats(s2),
            "out": out.detach(), "gelu_grad": gelu_grad, "d_ctx": d_ctx, "d_x": d_x, "d_h1": g[2], "d_h2": g[3], "d_h3": g[4],
            "dgb": torch.stack(g[5:9])}


# ---------------------------------------------------------------------------------------------------------------------------
# the six projections in front of the attention core
PROJ_MATS = ("q", "k", "v", "aq", "ak")


def proj_seq_len(rows):
    """L of the affine planes for a launch of `rows` rows: the largest divisor of rows that is <= 256 (rows = B * L)."""
    return max(d for d in range(1, min(rows, 256) + 1) if rows % d == 0)


def proj_case(H, G, rows, n_heads=2):
    """x, the six nn.Linear (scaled as in tests/test_hip_proj.py), the spatial calibrator's parameters, every cotangent."""
    g = _gen(H, G, rows)
    r = lambda *s: torch.randn(*s, generator=g)
    scale = 0.2 * (64 / H) ** 0.5
    dh = H // n_heads
    c = {"H": H, "G": G, "rows": rows, "n_heads": n_heads, "L": proj_seq_len(rows), "x": r(rows, H)}
    for n in PROJ_MATS:
        c["w" + n], c["b" + n] = scale * r(H, H), 0.1 * r(H)
    if G:
        c["wg"], c["bg"] = scale * r(G, H), 0.1 * r(G)
    c["w_order"], c["b_order"], c["w_dist"], c["b_dist"] = 0.3 * r(2 * dh), 0.1 * r(1), 0.3 * r(2 * dh), 0.1 * r(1)
    for k in ("dmq", "dmk", "dmv", "dqa", "dka", "dx_init"):
        c[k] = r(rows, H)
    c["dgate"] = r(rows, G) if G else None
    return c


def proj_fwd_ref(c):
    """mq, mk, mv, qa, ka, gate (logits), gate_prob (their sigmoid) and affine [B, nh, 4, LP] (padding entries zero: the
    kernel leaves them alone) of acattn_projections_fwd."""
    F = torch.nn.functional
    d = {k: v.double() for k, v in c.items() if isinstance(v, torch.Tensor)}
    H, nh, L, rows = c["H"], c["n_heads"], c["L"], c["rows"]
    dh, B, LP = H // nh, rows // L, 16 * ((L + 15) // 16)
    mq, mk, mv = F.linear(d["x"], d["wq"], d["bq"]), F.linear(d["x"], d["wk"], d["bk"]), F.linear(d["x"], d["wv"], d["bv"])
    out = {"mq": mq, "mk": mk, "mv": mv, "qa": F.linear(mq, d["waq"], d["baq"]), "ka": F.linear(mk, d["wak"], d["bak"])}
    if c["G"]:
        out["gate"] = F.linear(mq, d["wg"], d["bg"])
        out["gate_prob"] = torch.sigmoid(out["gate"])
    log2e = 1.4426950408889634
    qh, kh = mq.view(B, L, nh, dh).transpose(1, 2), mk.view(B, L, nh, dh).transpose(1, 2)  # [B, nh, L, dh]
    aff = torch.zeros(B, nh, 4, LP, dtype=torch.float64)
    aff[:, :, 0, :L] = -log2e * (qh @ d["w_order"][:dh] + d["b_order"])
    aff[:, :, 1, :L] = qh @ d["w_dist"][:dh] + d["b_dist"]
    aff[:, :, 2, :L] = -log2e * (kh @ d["w_order"][dh:])
    aff[:, :, 3, :L] = kh @ d["w_dist"][dh:]
    out["affine"] = aff
    return out


def proj_bwd_ref(c, given, dx_init):
    """dmq_total, dmk_total, dx of acattn_projections_bwd for the cotangents named in `given` (the others are zero)."""
    d = {k: v.double() for k, v in c.items() if isinstance(v, torch.Tensor)}
    z = torch.zeros(c["rows"], c["H"], dtype=torch.float64)
    cot = lambda k: d[k] if k in given else z
    qt = cot("dmq") + cot("dqa") @ d["waq"]
    if "dgate" in given and c["G"]:
        qt = qt + d["dgate"] @ d["wg"]
    kt = cot("dmk") + cot("dka") @ d["wak"]
    dx = qt @ d["wq"] + kt @ d["wk"] + cot("dmv") @ d["wv"]
    if dx_init:
        dx = dx + d["dx_init"]
    return {"dmq_total": qt, "dmk_total": kt, "dx": dx}
