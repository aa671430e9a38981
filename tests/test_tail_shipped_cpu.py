"""CPU suite: the layer tail's size queries at hidden 128 / inner 64, the shape of three of the four shipped dataset
configurations (yelp, amazon-sports-outdoors, amazon-toys-games).  Host-side answers of the built library only; nothing
is launched."""
import os
from types import SimpleNamespace

import pytest

from ac_tsr_amd import _lib, tail


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_hidden_128_inner_64_is_a_supported_pair(lib):
    assert lib.acattn_layer_tail_supported(128, 64) == 1
    assert lib.acattn_layer_tail_supported(96, 256) == 0


def test_backward_workspace_holds_the_three_transposed_matrices(lib):
    # W1^T [128][64], W2^T [64][128] and Wd^T [128][128]: the square one is the largest here
    assert lib.acattn_layer_tail_bwd_workspace_bytes(128, 64) == (2 * 128 * 64 + 128 * 128) * 4 == 131072


def test_one_partial_row_per_16_row_block(lib):
    assert lib.acattn_layer_tail_bwd_partial_rows_for(37, 128) == 3


def test_no_split_planes_at_hidden_128(lib):
    assert lib.acattn_layer_tail_split_bytes(128, 64, 512) == 0


def test_python_routes_the_pair_to_the_single_launch_node(lib):
    att = SimpleNamespace(dense=SimpleNamespace(out_features=128))
    ffn = SimpleNamespace(dense_1=SimpleNamespace(out_features=64))
    assert tail.fused_supported(att, ffn)
