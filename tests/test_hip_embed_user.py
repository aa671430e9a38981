"""GPU suite (-m gpu): the personalised front end dropout(LayerNorm(cat(E[idx], U[user] over L) + P)) of ACSSEPT
(acssept.py:120-131) against torch ops in fp64.  Tolerances of tests/test_hip_embed.py: forward <= 3e-5, each gradient
<= 1e-4 * max|g| + 1e-6."""
import pytest
import torch

from ac_tsr_amd import attn_launch, fused_embed, fused_embed_user

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (B, L, H, Di, items, users)
SHAPES = [(7, 37, 128, 64, 300, 11), (5, 7, 64, 32, 50, 4), (3, 50, 128, 96, 50, 3), (2, 17, 64, 16, 20, 2),
          (1, 1, 64, 32, 5, 2), (9, 50, 256, 128, 40, 5)]


def _modules(N, U, L, H, Di, with_pos, g):
    item = torch.nn.Embedding(N, Di, padding_idx=0)
    user = torch.nn.Embedding(U, H - Di, padding_idx=0)
    pos = torch.nn.Embedding(L + 3, H) if with_pos else None  # more rows than positions: only the first L are touched
    norm = torch.nn.LayerNorm(H, eps=1e-12)
    with torch.no_grad():
        item.weight.copy_(torch.randn(N, Di, generator=g))
        user.weight.copy_(torch.randn(U, H - Di, generator=g))
        if pos is not None:
            pos.weight.copy_(0.5 * torch.randn(L + 3, H, generator=g))
        norm.weight.copy_(1 + 0.3 * torch.randn(H, generator=g))
        norm.bias.copy_(0.3 * torch.randn(H, generator=g))
    return item, user, pos, norm


def _batch(B, L, N, U, g):
    """Item id 0 (the padding behind each sequence's length, and a whole-padding row when B allows), user id 0 when there is
    more than one sequence, and one user three times when there are at least four."""
    lens = torch.randint(1, L + 1, (B,), generator=g)
    idx = torch.randint(1, N, (B, L), generator=g) * (torch.arange(L)[None, :] < lens[:, None])
    idx[0, -1] = 0
    uid = torch.randint(1, U, (B,), generator=g)
    if B >= 2:
        uid[1] = 0
    if B >= 5:
        uid[2] = uid[3] = uid[4] = U - 1
    return idx, uid


def _reference(idx, uid, item, user, pos, norm, keep, p, cot):
    """fp64 torch ops of acssept.py:120-131 and their gradients (item, user, gamma, beta, [pos])."""
    L, H = idx.shape[1], norm.normalized_shape[0]
    Ed, Ud = item.weight.detach().double().requires_grad_(True), user.weight.detach().double().requires_grad_(True)
    Pd = pos.weight.detach().double().requires_grad_(True) if pos is not None else None
    wd, bd = norm.weight.detach().double().requires_grad_(True), norm.bias.detach().double().requires_grad_(True)
    x = torch.cat([Ed[idx], Ud[uid].unsqueeze(1).expand(-1, L, -1)], dim=-1) + (Pd[:L].unsqueeze(0) if pos is not None else 0)
    ref = torch.nn.functional.layer_norm(x, (H,), wd, bd, 1e-12)
    if keep is not None:
        ref = ref * keep.double() / (1 - p)
    grads = list(torch.autograd.grad((ref * cot.double()).sum(), [Ed, Ud, wd, bd] + ([Pd] if pos is not None else [])))
    grads[0][0] = 0  # nn.Embedding(padding_idx=0): the padding rows receive no gradient
    grads[1][0] = 0
    return ref.detach(), grads


@pytest.fixture(params=[True, False], ids=["sum_first", "scatter"])
def user_design(request, monkeypatch):
    """Both designs of the user-table gradient (fused_embed_user.USER_SUM_FIRST): summed over a sequence's positions first,
    or scattered per row."""
    monkeypatch.setattr(fused_embed_user, "USER_SUM_FIRST", request.param)
    return request.param


@pytest.mark.parametrize("B,L,H,Di,N,U", SHAPES)
@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_embed_user_layernorm_matches_torch(B, L, H, Di, N, U, with_pos, p, user_design):
    g = torch.Generator().manual_seed(B + L + H + Di)
    item, user, pos, norm = _modules(N, U, L, H, Di, with_pos, g)
    idx, uid = _batch(B, L, N, U, g)
    keep = torch.empty(B, L, H).bernoulli_(1 - p, generator=g) if p > 0 else None
    cot = torch.randn(B, L, H, generator=g)
    ref, grads = _reference(idx, uid, item, user, pos, norm, keep, p, cot)
    item_c, user_c, norm_c = item.to(DEV), user.to(DEV), norm.to(DEV)
    pos_c = pos.to(DEV) if with_pos else None
    y, nonzero = fused_embed_user.embed_user_layer_norm(idx.to(DEV), uid.to(DEV), item_c, user_c, pos_c, norm_c, p,
                                                        training=False, keep=None if keep is None else keep.to(DEV),
                                                        return_nonzero=True)
    assert y.shape == (B, L, H)
    assert (y.detach().cpu() - ref.float()).abs().max() <= 3e-5
    assert nonzero.dtype == torch.uint8 and torch.equal(nonzero.cpu(), (idx != 0).to(torch.uint8))
    got = torch.autograd.grad((y * cot.to(DEV)).sum(), [item_c.weight, user_c.weight, norm_c.weight, norm_c.bias] +
                              ([pos_c.weight] if with_pos else []))
    for name, a, b in zip(("item", "user", "gamma", "beta", "pos"), got, grads):
        assert a.shape == b.shape, name
        assert (a.cpu() - b.float()).abs().max() <= 1e-4 * b.abs().max() + 1e-6, name
    assert got[0][0].abs().max() == 0 and got[1][0].abs().max() == 0  # the padding rows: exactly zero
    if with_pos:
        assert got[4][L:].abs().max() == 0


def test_repeated_user_collects_every_sequence(user_design):
    """Correctness does not depend on the users of a batch being distinct: every sequence has the SAME user."""
    B, L, H, Di, N, U = 12, 50, 128, 64, 30, 3
    g = torch.Generator().manual_seed(5)
    item, user, pos, norm = _modules(N, U, L, H, Di, True, g)
    idx, _ = _batch(B, L, N, U, g)
    uid = torch.full((B,), 2, dtype=torch.long)
    cot = torch.randn(B, L, H, generator=g)
    _, grads = _reference(idx, uid, item, user, pos, norm, None, 0.0, cot)
    item_c, user_c, pos_c, norm_c = item.to(DEV), user.to(DEV), pos.to(DEV), norm.to(DEV)
    y = fused_embed_user.embed_user_layer_norm(idx.to(DEV), uid.to(DEV), item_c, user_c, pos_c, norm_c, 0.0, training=False)
    d_user, = torch.autograd.grad((y * cot.to(DEV)).sum(), [user_c.weight])
    assert (d_user.cpu() - grads[1].float()).abs().max() <= 1e-4 * grads[1].abs().max() + 1e-6
    assert d_user[:2].abs().max() == 0 and d_user[2].abs().max() > 0


def test_counter_dropout_statistics_and_bad_ids():
    g = torch.Generator().manual_seed(0)
    B, L, H, Di, N, U = 256, 50, 128, 64, 1000, 40
    item, user, pos, norm = (m.to(DEV) for m in _modules(N, U, L, H, Di, True, g))
    idx = torch.randint(1, N, (B, L), generator=g).to(DEV)
    uid = torch.randint(1, U, (B,), generator=g).to(DEV)
    torch.manual_seed(1)
    a = fused_embed_user.embed_user_layer_norm(idx, uid, item, user, pos, norm, 0.5, training=True)
    b = fused_embed_user.embed_user_layer_norm(idx, uid, item, user, pos, norm, 0.5, training=True)
    e = fused_embed_user.embed_user_layer_norm(idx, uid, item, user, pos, norm, 0.5, training=False)
    zero_a, zero_b = (a == 0).float().mean().item(), (b == 0).float().mean().item()
    assert abs(zero_a - 0.5) < 0.01 and abs(zero_b - 0.5) < 0.01 and not torch.equal(a == 0, b == 0)
    kept = a != 0
    assert (a[kept] - 2 * e[kept]).abs().max() <= 1e-5  # survivors are scaled by 1 / (1 - p)
    # ids outside either table are clamped, not dereferenced
    bad, bad_u = idx.clone(), uid.clone()
    bad[0, 0], bad[0, 1] = N + 12345, -7
    bad_u[0], bad_u[1] = U + 999, -3
    out = fused_embed_user.embed_user_layer_norm(bad, bad_u, item, user, pos, norm, 0.0, training=False)
    assert torch.isfinite(out).all()
    d_item, d_user = torch.autograd.grad(out.sum(), [item.weight, user.weight])
    assert torch.isfinite(d_item).all() and torch.isfinite(d_user).all()
    with pytest.raises(IndexError):
        fused_embed_user.embed_user_layer_norm(torch.ones(2, L + 4, dtype=torch.long, device=DEV),
                                               torch.ones(2, dtype=torch.long, device=DEV), item, user, pos, norm, 0.0, False)


def test_constant_user_equals_the_item_only_front_end():
    """H = 64, Di = 32, every user row the same vector u: the forward is fused_embed.embed_layer_norm on a 64-wide table whose
    rows are [item_row | u], to 1e-6."""
    B, L, H, Di, N, U = 5, 23, 64, 32, 50, 4
    g = torch.Generator().manual_seed(9)
    item, user, pos, norm = _modules(N, U, L, H, Di, True, g)
    with torch.no_grad():
        user.weight.copy_(user.weight[1].expand(U, -1).clone())
    idx, uid = _batch(B, L, N, U, g)
    wide = torch.nn.Embedding(N, H, padding_idx=0)
    with torch.no_grad():
        wide.weight.copy_(torch.cat([item.weight, user.weight[:1].expand(N, -1)], dim=1))
    item, user, pos, norm, wide = (m.to(DEV) for m in (item, user, pos, norm, wide))
    a = fused_embed_user.embed_user_layer_norm(idx.to(DEV), uid.to(DEV), item, user, pos, norm, 0.0, training=False)
    b = fused_embed.embed_layer_norm(idx.to(DEV), wide, pos, norm, 0.0, training=False)
    assert (a - b).abs().max() <= 1e-6


def test_every_output_is_written_under_poison(monkeypatch, user_design):
    """attn_launch.POISON: the outputs start as NaN, so an element a kernel does not write stays NaN."""
    monkeypatch.setattr(attn_launch, "POISON", True)
    B, L, H, Di, N, U = 7, 37, 128, 64, 300, 11
    g = torch.Generator().manual_seed(2)
    item, user, pos, norm = (m.to(DEV) for m in _modules(N, U, L, H, Di, True, g))
    idx, uid = _batch(B, L, N, U, g)
    y = fused_embed_user.embed_user_layer_norm(idx.to(DEV), uid.to(DEV), item, user, pos, norm, 0.0, training=False)
    assert torch.isfinite(y).all()
    got = torch.autograd.grad((y * torch.randn(B, L, H, generator=g).to(DEV)).sum(),
                              [item.weight, user.weight, pos.weight, norm.weight, norm.bias])
    for t in got:
        assert torch.isfinite(t).all()


def test_item_table_gradient_hand_over_and_attack_pass():
    """The item half joins StepState's table-gradient hand-over exactly as fused_embed does: inside the calibrated pass the
    cross-entropy node's published [n_items, Di] gradient receives the scattered rows; same numbers as autograd's sum
    outside a pass.  In the attack pass the node returns nothing."""
    from ac_tsr_amd import ce
    from ac_tsr_amd.state import StepState
    B, L, H, Di, N, U = 16, 12, 128, 64, 300, 9
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, N, (B, L), generator=g).to(DEV)
    uid = torch.randint(0, U, (B,), generator=g).to(DEV)
    target = torch.randint(1, N, (B,), generator=g).to(DEV)
    cot = torch.randn(B, L, H, generator=g).to(DEV)

    def grads(state, mode):
        torch.manual_seed(0)
        item = torch.nn.Embedding(N, Di, padding_idx=0).to(DEV)
        user = torch.nn.Embedding(U, H - Di, padding_idx=0).to(DEV)
        norm = torch.nn.LayerNorm(H, eps=1e-12).to(DEV)
        if state is not None:
            for m in (item, user, norm):
                state.attach(m)
        kw = {} if state is None else {"state": state}
        y = fused_embed_user.embed_user_layer_norm(idx, uid, item, user, None, norm, 0.0, training=True)
        loss = ce.full_sort_cross_entropy(y[:, -1, :Di], item.weight, target, **kw) + (y * cot).sum() * 1e-2
        if mode == "calibrated":
            with state.calibrated_pass():
                loss.backward()
        elif mode == "attack":
            with state.attack_pass():
                ((y * cot).sum()).backward()
        else:
            loss.backward()
        return item.weight.grad, user.weight.grad, norm.weight.grad

    # the two runs add the same fp32 terms to an address in a different order (float atomics): at most B * L = 192 terms per
    # address, each rounding within 2^-24 of the running sum -> 192 * 2^-24 = 1.2e-5 of the gradient's scale at worst; rows
    # lost to a broken hand-over would be off by the scale itself
    close = lambda a, b: (a - b).abs().max() <= 1.2e-5 * a.abs().max() + 1e-9
    ref = grads(None, None)
    st = StepState()
    got = grads(st, "calibrated")
    assert st.table_grad is None  # published and taken
    assert all(close(a, b) for a, b in zip(ref, got))
    assert all(t is None for t in grads(StepState(), "attack"))
