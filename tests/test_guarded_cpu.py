"""CPU suite: the guarded-buffer helper of the row-edge tests (tests/_guarded.py) on CPU tensors, and the fp64 references of
tests/_row_edge_refs.py at the smallest shape of each family: each must be finite wherever the GPU tests demand "no poison",
so that the demand is one the reference alone meets."""
import pytest
import torch

from tests import _row_edge_refs as R
from tests._guarded import _POISON, ALIGN, MIN_GUARD_ELEMS, MIN_GUARD_ROWS, guard_elems, guarded

DTYPES = [torch.float32, torch.uint8, torch.int64]


def _one(dtype):
    return torch.ones((), dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_width", [2, 50, 64, 130, 1024])
def test_layout_and_alignment(dtype, row_width):
    for rows in (1, 3, 17):
        g = guarded((rows, row_width), dtype, "cpu", row_width, "poison")
        assert g.t.shape == (rows, row_width) and g.t.dtype == dtype and g.t.is_contiguous()
        assert g.t.data_ptr() % ALIGN == 0
        n = guard_elems(row_width, dtype)
        assert n >= MIN_GUARD_ROWS * row_width and n >= MIN_GUARD_ELEMS and (n * g.t.element_size()) % ALIGN == 0
        # both guards lie inside the one allocation, in front of and behind the payload
        esz = g.t.element_size()
        first = (g.t.data_ptr() - g.flat.data_ptr()) // esz
        assert first >= n and g.flat.numel() - first - g.t.numel() >= n
        g.t.copy_(torch.zeros(rows, row_width, dtype=dtype))
        g.check("clean")


@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_write_passes_and_unwritten_element_fails(dtype):
    g = guarded((5, 6), dtype, "cpu", 6, "poison")
    with pytest.raises(AssertionError, match=r"out: poison left .* offset 0 = index \(0, 0\) \(30 of 30"):
        g.check("out")
    g.t.fill_(1)
    g.check("out")
    g = guarded((5, 6), dtype, "cpu", 6, "poison")
    g.t.fill_(1)
    g.bits[g.start + 13] = _POISON[dtype]
    with pytest.raises(AssertionError, match=r"out: poison left .* offset 13 = index \(2, 1\) \(1 of 30"):
        g.check("out")


def test_poison_is_the_allocators_nan():
    g = guarded((4,), torch.float32, "cpu", 1, "poison")
    want = torch.full((4,), float("nan")).view(torch.int32)
    assert torch.equal(g.t.view(torch.int32), want)
    assert bool(torch.isnan(g.flat).all())  # the guards are NaNs too (what a read past an input's last row finds) ...
    assert not bool((g.bits[:g.start] == want[0]).any())  # ... of another bit pattern


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", ["poison", "zero", "input"])
def test_store_one_element_outside_the_payload_fails(dtype, fill):
    def fresh():
        g = guarded((3, 7), dtype, "cpu", 7, torch.ones(3, 7, dtype=dtype) if fill == "input" else fill)
        g.t.fill_(1)
        g.check("buf")
        return g
    g = fresh()
    g.flat[g.start - 1] = _one(dtype)
    with pytest.raises(AssertionError, match=r"dq: front guard overwritten at payload offset -1 \(1 elements"):
        g.check("dq")
    g = fresh()
    g.flat[g.start + 21] = _one(dtype)
    with pytest.raises(AssertionError, match=r"dq: back guard overwritten at payload offset 21 \(1 elements"):
        g.check("dq")
    g = fresh()  # a whole row block behind the end: 64 rows further the guard still stands
    g.flat[g.start + 21 + 63 * 7:g.start + 21 + 64 * 7] = _one(dtype)
    with pytest.raises(AssertionError, match=rf"dq: back guard overwritten at payload offset {21 + 63 * 7} \(7 elements"):
        g.check("dq")
    g = fresh()  # the guard's own value written back is not a store the bits can show; any other NaN is
    if dtype == torch.float32:
        g.flat[g.start + 22] = float("nan")
        with pytest.raises(AssertionError, match=r"back guard overwritten at payload offset 22"):
            g.check("dq")


def test_unwritten_exempts_exactly_its_mask():
    g = guarded((4, 8), torch.float32, "cpu", 8, "poison")
    g.t[:, :6] = 2.0
    mask = torch.zeros(4, 8, dtype=torch.bool)
    mask[:, 6:] = True
    g.check("affine", unwritten=mask)
    mask[3, 7] = False  # one element fewer exempt: that element fails
    with pytest.raises(AssertionError, match=r"affine: poison left .* offset 31 = index \(3, 7\) \(1 of 32"):
        g.check("affine", unwritten=mask)
    g.t[3, 7] = 0.0
    g.t[0, 0] = float("nan")  # an element outside the mask is not exempt, whatever the mask covers
    with pytest.raises(AssertionError, match=r"affine: .* offset 0 = index \(0, 0\)"):
        g.check("affine", unwritten=mask)
    with pytest.raises(AssertionError, match="may not cover the whole tensor"):
        g.check("affine", unwritten=torch.ones(4, 8, dtype=torch.bool))
    z = guarded((4, 8), torch.float32, "cpu", 8, "zero")
    with pytest.raises(AssertionError, match="only applies to poisoned outputs"):
        z.check("d_table", unwritten=mask)


def test_inputs_keep_their_bits_and_end_in_a_nan_or_an_out_of_range_id():
    x = torch.randn(3, 4)
    g = guarded((3, 4), torch.float32, "cpu", 4, x)
    assert torch.equal(g.t, x) and bool(torch.isnan(g.flat[g.start + 12:]).all())
    g.check("x")
    g.t[1, 1] += 1
    with pytest.raises(AssertionError, match="x: input overwritten at payload offset 5"):
        g.check("x")
    ids = torch.arange(5)
    gi = guarded((5,), torch.int64, "cpu", 1, ids)
    assert int(gi.flat[gi.start + 5]) > 2 ** 40  # an id outside every table
    gi.check("idx")
    z = guarded((3, 4), torch.float32, "cpu", 4, "zero")
    assert float(z.t.abs().max()) == 0
    z.t[2, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"d_table: NaN at payload offset 11 = index \(2, 3\)"):
        z.check("d_table")


# ---------------------------------------------------------------------------------------------------------------------------
def _finite(ref):
    for name, t in ref.items():
        assert t.dtype in (torch.float64, torch.uint8), name
        assert bool(torch.isfinite(t.double()).all()), name


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_ln_reference_is_finite(H, p):
    c = R.ln_case(H, 1, 1, p)
    ref = R.ln_ref(c)
    _finite(ref)
    assert ref["y"].shape == (1, H) and ref["stats"].shape == (1, 2) and ref["dz"].shape == ref["dres"].shape == (1, H)
    c = R.ln_case(H, 3 * (R.rpb(H) + 1), R.rpb(H) + 1, p)
    _finite(R.ln_ref(c))
    # against torch's own fp32 path: the reference is the operation the existing tests name
    y32 = torch.nn.functional.layer_norm(
        c["z"] * (c["keep"].float() / (1 - p) if p > 0 else 1.0) + c["residual"].repeat(3, 1), (H,), c["gamma"], c["beta"], 1e-12)
    assert (y32.double() - R.ln_ref(c)["y"]).abs().max() <= 2e-5


def test_ln_row_list_matches_the_launch_geometry():
    assert [R.rpb(H) for H in (64, 128, 256)] == [16, 8, 4]
    assert R.ln_rows(64) == [1, 15, 16, 17, 8191, 8193, 32767, 32768, 32769, 65539]
    assert max(R.ln_rows(256)) == 16387 and max(R.ln_rows(128)) == 32771


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_embed_references_are_finite(H, p):
    for B, L in ((1, 1), (5, 3)):
        c = R.embed_case(H, B, L, 7, p)
        ref = R.embed_ref(c)
        _finite(ref)
        assert ref["d_table"].shape == (7, H) and ref["d_pos"].shape == (L, H) and ref["nonzero"].shape == (B * L,)
        assert float(ref["d_table"][0].abs().max()) == 0  # the padding row
        for Di in (4, H // 2, H - 4):
            cu = R.embed_user_case(H, Di, B, L, 7, 3, p)
            ru = R.embed_user_ref(cu)
            _finite(ru)
            assert ru["d_item"].shape == (7, Di) and ru["d_user"].shape == (3, H - Di) and ru["user_rows"].shape == (B * L, H - Di)
    # clamped ids: -1 reads (and, being the padding row, skips) row 0, N reads and accumulates into row N - 1
    c = R.embed_case(H, 5, 3, 7, p)
    assert c["idx"].view(-1)[0] == -1 and c["idx"].view(-1)[1] == 7 and c["idx"].view(-1)[-1] == 6
    assert R.embed_ref(c)["nonzero"][0] == 1


def test_small_reduction_references_are_finite():
    assert torch.equal(R.sum_rows_ref(torch.ones(2, 3, 4)), torch.full((2, 4), 3.0, dtype=torch.float64))
    c = R.dense_ce_case(1, 1)
    ref = R.dense_ce_ref(c)
    _finite(ref)
    assert float(ref["row_loss"].abs().max()) == 0 and float(ref["d_logits"].abs().max()) == 0  # one class: p = 1
    c = R.dense_ce_case(3, 257)
    ref = R.dense_ce_ref(c)
    _finite(ref)
    want = torch.nn.functional.cross_entropy(c["logits"].double(), c["target"], reduction="none")
    assert (ref["row_loss"] - want).abs().max() <= 1e-12
    m = torch.rand(2, 2, 17, 17)
    pen = R.penalty_rows_ref(m)
    assert pen.shape == (2, 2, 2) and abs(float(pen.sum()) - float(((1 - m.double()) ** 2).sum())) <= 1e-9


@pytest.mark.parametrize("H,I", [(64, 128), (64, 256), (128, 64), (256, 1024)])
@pytest.mark.parametrize("pick", [False, True])
def test_tail_reference_is_finite(H, I, pick):
    for rows, p in ((1, 0.0), (3, 0.5)):
        c = R.tail_case(H, I, rows, p, pick)
        ref = R.tail_ref(c)
        _finite(ref)
        assert ref["act"].shape == ref["gelu_grad"].shape == ref["d_h2"].shape == (rows, I)
        assert ref["d_ctx"].shape == ref["d_x"].shape == c["ctx"].shape and ref["dgb"].shape == (4, H)
    # gelu'(h) is the derivative of torch's erf-GELU
    h = torch.linspace(-4, 4, 33, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.nn.functional.gelu(h).sum(), [h])
    hd = h.detach()
    mine = 0.5 * (1 + torch.erf(hd / 2 ** 0.5)) + hd * torch.exp(-0.5 * hd * hd) / (2 * torch.pi) ** 0.5
    assert (g - mine).abs().max() <= 1e-12
    if pick:  # a position picked twice receives both rows' gradients; positions -1 and L are clamped into the sequence
        c = R.tail_case(H, I, 6, 0.5, True)
        src = R.tail_source_rows(c)
        assert src[0] == src[1] and int(src.min()) >= 0 and int(src.max()) < c["src_rows"]
        assert int(c["src_index"].min()) == -1 and int(c["src_index"].max()) == c["src_L"]


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("G", [0, 37, 200])
def test_projection_references_are_finite(H, G):
    c = R.proj_case(H, G, 1)
    fwd = R.proj_fwd_ref(c)
    _finite(fwd)
    assert fwd["affine"].shape == (1, 2, 4, 16) and float(fwd["affine"][..., 1:].abs().max()) == 0
    c = R.proj_case(H, G, 34)
    assert c["L"] == 34
    fwd = R.proj_fwd_ref(c)
    _finite(fwd)
    assert fwd["affine"].shape == (1, 2, 4, 48)
    for given in (("dmq", "dmk", "dmv", "dqa", "dka", "dgate"), ("dqa", "dka"), ("dmq", "dmk", "dmv")):
        _finite(R.proj_bwd_ref(c, given, True))
    # against autograd through the same six linears
    x = c["x"].double().requires_grad_(True)
    lin = torch.nn.functional.linear
    mq, mk, mv = (lin(x, c["w" + n].double(), c["b" + n].double()) for n in ("q", "k", "v"))
    loss = (mq * c["dmq"].double()).sum() + (mk * c["dmk"].double()).sum() + (mv * c["dmv"].double()).sum() \
        + (lin(mq, c["waq"].double(), c["baq"].double()) * c["dqa"].double()).sum() \
        + (lin(mk, c["wak"].double(), c["bak"].double()) * c["dka"].double()).sum()
    if G:
        loss = loss + (lin(mq, c["wg"].double(), c["bg"].double()) * c["dgate"].double()).sum()
    (dx,) = torch.autograd.grad(loss, [x])
    assert (dx - R.proj_bwd_ref(c, ("dmq", "dmk", "dmv", "dqa", "dka", "dgate"), False)["dx"]).abs().max() <= 1e-10


def test_cross_entropy_and_weight_gradient_references_are_finite():
    from tests import test_hip_row_edges_ce as ce_mod
    from tests import test_hip_row_edges_linear as lin_mod
    c, ref = ce_mod._case(1, 64)
    _finite(ref)
    assert ref["d_table"].shape == (64, 64) and ref["dir"].shape == (1, 64)
    want = torch.nn.functional.cross_entropy(c["out"].double() @ c["table"].double().t(), c["target"], reduction="none")
    assert (ref["row_loss"] - want).abs().max() <= 1e-12
    x, dy, dw, db = lin_mod._case(1, 64, 50)
    assert dw.shape == (50, 64) and db.shape == (50,) and bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
