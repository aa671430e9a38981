"""GPU suite (-m gpu): whole models at the shipped hidden 128 / inner 64 shapes -- `model_yelp` (3 layers, 8 heads, eval) and
`model_sports` (2 layers, 2 heads, training mode with every dropout mask handed over), fixtures the genuine reference
produced (tools/gen_shipped_golden.py) -- through the bodies and thresholds of the existing model tests, with the unfused
tail node made to raise: the single-launch node (acattn_layer_tail_fwd / _bwd) must have served every layer, the last
layer's picked rows included.

A fixture at hidden 128 is several MB and is committed in parts under 1 MiB, tests/golden/<name>.partNN.npz, each holding
some of the arrays under their own keys; `golden_dir` writes them back into one <name>.npz for `Case(name)`."""
import glob
import os

import numpy as np
import pytest

from ac_tsr_amd import tail
from tests import _golden
from tests.test_hip_backward import test_two_pass_trainer_gradients_match_reference as _two_pass
from tests.test_hip_combined import test_one_walk_gives_the_reference_gradients as _one_walk
from tests.test_hip_forward import test_model_logits_within_1e4 as _logits

pytestmark = pytest.mark.gpu
NAMES = ["model_sports", "model_yelp"]


@pytest.fixture(scope="module")
def golden_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("shipped_golden")
    for name in NAMES:
        parts = sorted(glob.glob(os.path.join(_golden.GOLDEN_DIR, name + ".part*.npz")))
        assert parts, name
        arrays = {}
        for path in parts:
            z = np.load(path, allow_pickle=False)
            assert not set(z.files) & set(arrays), path
            arrays.update({k: z[k] for k in z.files})
        np.savez(os.path.join(str(d), name + ".npz"), **arrays)
    return str(d)


@pytest.fixture
def fused_only(golden_dir, monkeypatch):
    """`Case(name)` finds the two fixtures, and the hipBLASLt / ATen tail node is unreachable."""
    monkeypatch.setattr(_golden, "GOLDEN_DIR", golden_dir)

    def unreachable(*args, **kwargs):
        raise AssertionError("the unfused tail node ran at hidden 128 / inner 64")

    monkeypatch.setattr(tail._LayerTail, "apply", unreachable)


def test_yelp_logits_within_1e4(fused_only):
    _logits("model_yelp")


@pytest.mark.parametrize("prune", [True, False], ids=["pruned_schedule", "reference_schedule"])
@pytest.mark.parametrize("name", NAMES)
def test_two_pass_gradients_with_the_fused_tail_only(fused_only, name, prune):
    _two_pass(name, prune_dead_work=prune)


@pytest.mark.parametrize("prune", [True, False], ids=["pruned_schedule", "reference_schedule"])
@pytest.mark.parametrize("name", NAMES)
def test_one_walk_gradients_with_the_fused_tail_only(fused_only, name, prune):
    _one_walk(name, prune)
