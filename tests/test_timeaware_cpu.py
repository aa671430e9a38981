"""CPU suite of the ACTiSASRec feature: the restatement tests/_timeaware_ref.py against the committed fixtures of the genuine
reference (tests/golden/tisasrec_*, tools/gen_tisasrec_golden.py), the model's state-dict surface, get_time_matrix, the
padding-row rule, the restatement's reduction to tests/_unnorm_ref.py, the C layout of the new structs and the limits
acattn_timeaware_attention_supported names -- nothing here launches a kernel."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import ac_tsr_amd as A
from ac_tsr_amd import _lib
from oracle import ac_tsr_ref as O
from tests import _attention_fp64 as F
from tests import _timeaware_cases as TC
from tests import _timeaware_ref as T
from tests import _unnorm_ref as U
from tests._tisasrec_golden import TisasrecCase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TWO_PASS = {}


def _two_pass(name):
    """(case, att_loss, cal_loss, grads with row 0 zeroed, un-masked grads) of the restatement on a fixture, once."""
    if name not in _TWO_PASS:
        c = TisasrecCase(name)
        args = (c.batch(), c.params(), c.model_cfg(), c.span, c.layer_randomness(), c.model_randomness())
        att, cal, grads = T.two_pass_grads(*args)
        _, _, plain = T.two_pass_grads(*args, zero_padding_rows=False)
        _TWO_PASS[name] = (c, att, cal, grads, plain)
    return _TWO_PASS[name]


@pytest.mark.parametrize("name", ["tisasrec_train", "tisasrec_eval"])
def test_restatement_reproduces_the_two_pass_run_of_the_reference(name):
    c, att, cal, grads, _ = _two_pass(name)
    assert abs(att.item() - float(c.raw["out.att_loss"])) <= 2e-5
    assert abs(cal.item() - float(c.raw["out.cal_loss"])) <= 2e-5
    ref = c.grads()
    assert set(ref) == set(grads)
    for n, g in ref.items():
        assert (grads[n] - g).abs().max().item() <= 2e-3 * max(g.abs().max().item(), 1e-6), n


def test_restatement_reproduces_the_full_sort_scores_of_the_reference():
    c = TisasrecCase("tisasrec_eval")
    with torch.no_grad():
        att, cal = T.full_sort_predict(c.batch(), c.params(), c.model_cfg(), c.span, c.layer_randomness("score_noise"))
    assert (att - c.t("out.attacked_scores")).abs().max() <= 2e-5
    assert (cal - c.t("out.scores")).abs().max() <= 2e-5


@pytest.mark.parametrize("name", ["tisasrec_train", "tisasrec_eval"])
def test_state_dict_keys_are_the_references_and_the_fixture_loads(name):
    c = TisasrecCase(name)
    model = A.ACTiSASRec(A.DictConfig(c.config()), A.ItemCount(c.n_items))
    assert set(model.state_dict()) == set(c.params())
    model.load_state_dict(c.params(), strict=True)
    for k, v in c.params().items():
        assert torch.equal(model.state_dict()[k], v), k
    assert model.timestamp == "timestamp_list" and model.time_span == c.span
    assert model.time_matrix_emb_K_embedding.padding_idx == 0 and model.absolute_pos_V_embedding.padding_idx == 0


def test_get_time_matrix_on_equal_far_apart_and_padded_stamps():
    cfg = dict(TisasrecCase("tisasrec_eval").config(), MAX_ITEM_LIST_LENGTH=4, time_span=10)
    model = A.ACTiSASRec(A.DictConfig(cfg), A.ItemCount(20))
    stamps = torch.tensor([[5, 5, 8, 100], [7, 9, 0, 0]])  # equal, near, far apart; right padding (stamp 0)
    got = model.get_time_matrix(stamps)
    want = torch.tensor([[[0, 0, 3, 10], [0, 0, 3, 10], [3, 3, 0, 10], [10, 10, 10, 0]],
                         [[0, 2, 7, 7], [2, 0, 9, 9], [7, 9, 0, 0], [7, 9, 0, 0]]], dtype=torch.int32)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    assert torch.equal(got, T.get_time_matrix(stamps, 10))
    c = TisasrecCase("tisasrec_train")
    big = A.ACTiSASRec(A.DictConfig(c.config()), A.ItemCount(c.n_items))
    tm = big.get_time_matrix(c.batch()["timestamp_list"])
    assert torch.equal(tm, T.get_time_matrix(c.batch()["timestamp_list"], c.span))
    off = ~torch.eye(c.L, dtype=torch.bool).expand_as(tm)
    assert (tm[off] == 0).any() and (tm == c.span).any()  # the fixture reaches row 0 off the diagonal and the clip
    assert sorted(c.batch()["item_length"].tolist())[0] == 1 and c.L in c.batch()["item_length"].tolist()


def test_the_fixture_exercises_the_padding_row_rule():
    """Row 0 of the four padded tables: zero in the reference's gradients (nn.Embedding(padding_idx=0)), although the forward
    reads those rows (the reference's initialisation overwrites them) and their un-masked derivative is not zero."""
    c, _, _, grads, plain = _two_pass("tisasrec_train")
    ref = c.grads()
    for n in T.PADDED_TABLES:
        assert c.params()[n][0].abs().max() > 0, n   # row 0 is not a zero row
        assert ref[n][0].abs().max() == 0 and grads[n][0].abs().max() == 0, n
        assert plain[n][0].abs().max() > 1e-3 * plain[n].abs().max(), n
        assert torch.equal(plain[n][1:], grads[n][1:]), n


@pytest.mark.parametrize("shape,kw", [((3, 17, 32, 2), {}), ((2, 50, 128, 2), {"left_pad": True}), ((2, 33, 64, 2), {"causal": False})])
def test_with_zero_tables_the_restatement_is_the_unnormalised_core(shape, kw):
    base = F._case("zero_tables", "timeaware", shape, **kw)
    c = TC.TCase("zero_tables", base, 7, 0.5, TC.OUTPUTS, "mixed")
    p, draws = TC.problem(c), F.torch_draws(base)
    for k in TC.TIME_LEAVES:
        p.t[k].zero_()
    _, got = TC.oracle(c, p, draws, {}, torch.float64)
    with F.default_dtype(torch.float64):
        x = {k: v.double() for k, v in p.t.items()}
        cfg = O.EncoderCfg(n_layers=1, n_heads=base.nh, hidden_size=base.H, inner_size=4 * base.H, combine_option="gate",
                           seq_length=base.L, attn_dropout_prob=base.p_drop)
        ref = U.core_from_projected_unnorm(x["q"], x["k"], x["v"], x["qa"], x["ka"], x["gl"], p.mask_for_oracle.double(),
                                           x["w_order"], x["b_order"], x["w_dist"], x["b_dist"], x["scalar"], cfg,
                                           draws["noise"].double(), keep_after=draws["keep_after"].double(),
                                           keep_mask=draws["keep_mask"].double())
    for k in TC.OUTPUTS:
        assert F.err(got[k], ref[k]) <= 1e-12, k


def test_ctypes_layout_of_the_new_structs_matches_c(tmp_path):
    fields = {"acattn_time_ext": _lib.TimeExt, "acattn_time_grads": _lib.TimeGrads}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "acattn.h"', 'int main(void){']
    for cname, cls in fields.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(l.split() for l in out.strip().splitlines())
    for cname, cls in fields.items():
        assert int(got[cname]) == C.sizeof(cls)
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_supported_answers_without_a_gpu_and_names_each_limit():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()

    def ask(span=256, p_time=0.5, **kw):
        p, t = _lib.Problem(), _lib.TimeExt()
        p.B, p.L, p.H, p.n_heads, p.adversarial, p.two_level = 4, 50, 64, 2, 1, 1
        p.combine_option, p.mask_mode, p.rng_mode, p.p_drop = _lib.COMBINE["gate"], _lib.MASK_STRUCTURED, _lib.RNG_COUNTER, 0.5
        for k, v in kw.items():
            setattr(p, k, v)
        t.time_span, t.p_time = span, p_time
        ok = lib.acattn_timeaware_attention_supported(C.byref(p), C.byref(t))
        return ok, lib.acattn_last_error().decode()

    assert ask()[0] == 1
    for H in (32, 64, 128):  # head sizes 16, 32, 64 at the reference's default span
        assert ask(H=H)[0] == 1 and ask(H=H, span=1)[0] == 1
    assert ask(span=319, H=128)[0] == 1 and ask(span=1279, H=32)[0] == 1  # what the LDS plan takes
    for kw, text in ((dict(L=65), "L must be <= 64"), (dict(H=256), "head size"), (dict(H=16), "head size"),
                     (dict(combine_option=_lib.COMBINE["fixed"]), "gate"), (dict(two_level=0), "two_level"),
                     (dict(mask_mode=_lib.MASK_DENSE_LL), "structured"), (dict(adversarial=0), "adversarial"),
                     (dict(span=0), "time_span must be >= 1"), (dict(span=320, H=128), "160 KiB"), (dict(p_time=1.0), "p_time"),
                     (dict(p_drop=1.0), "p_drop"), (dict(rng_mode=7), "rng_mode")):
        ok, why = ask(**kw)
        assert ok == 0 and text in why, (kw, why)
    # a launch outside the domain is refused before any HIP call: -1 and the same text, never another kernel
    p, t, out = _lib.Problem(), _lib.TimeExt(), _lib.FwdOut()
    p.B, p.L, p.H, p.n_heads, p.adversarial, p.two_level, p.combine_option = 4, 65, 64, 2, 1, 1, _lib.COMBINE["gate"]
    t.time_span = 256
    assert lib.acattn_timeaware_attention_fwd(C.byref(p), C.byref(t), C.byref(out), None) == -1
    assert "L must be <= 64" in lib.acattn_last_error().decode()
    io, g = _lib.BwdIO(), _lib.TimeGrads()
    assert lib.acattn_timeaware_attention_bwd(C.byref(p), C.byref(t), C.byref(io), C.byref(g), None) == -1
    assert lib.acattn_time_rng_materialize(0, 5, 64, 1, 0.5, None, None, None) == -1


def test_the_operator_refuses_cpu_tensors_by_name():
    x = {k: torch.zeros(2, 8, 32) for k in ("q", "k", "v", "qa", "ka", "pos_k", "pos_v")}
    idx = torch.zeros(2, 8, 8, dtype=torch.int32)
    tab = torch.zeros(5, 32)
    with pytest.raises(ValueError, match="GPU"):
        A.timeaware_attention(x["q"], x["k"], x["v"], x["qa"], x["ka"], torch.zeros(2, 8, 8),
                              A.StructuredMask(torch.ones(2, 8, dtype=torch.uint8)), A.AttentionConfig(n_heads=2),
                              w_order=torch.zeros(1, 32), b_order=torch.zeros(1), w_dist=torch.zeros(1, 32), b_dist=torch.zeros(1),
                              scalar=torch.zeros(1), pos_k=x["pos_k"], pos_v=x["pos_v"], time_k=A.TimeIntervals(tab, idx),
                              time_v=A.TimeIntervals(tab, idx), seed=1)
