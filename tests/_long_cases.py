"""The case table of the long-sequence attention tests (tests/test_long_sequence_cases_cpu.py checks its conditioning on the
CPU, tests/test_hip_long_sequences.py runs it on the GPU): tests._attention_fp64.Case entries above the 208 keys the
row-resident kernels hold.  Nothing here touches a GPU or imports the HIP package.

Why these lengths: 209 is one key and one query row into key tile 14; 257 one row into tile 17, past a fourth group of 64
keys; 224 and 272 are whole tile counts; 300 is ragged in the last group of four; 496 is the ceiling
(acattn_max_sequence_length()).  Every batch but the single-sequence ones holds a second, shorter sequence, so whole key
tiles are empty; `left_pad` turns sequence 1 into one whose first rows see no key at all."""
from tests import _attention_fp64 as F


def _table():
    c = F._case
    return [
        c("dh32_L209", "train", (2, 209, 64, 2)),
        c("dh16_L257", "train", (2, 257, 64, 4)),
        c("dh32_L224_bidir_p0", "train", (2, 224, 64, 2), causal=False, p_drop=0.0),
        c("dh64_L300_bidir", "train", (1, 300, 128, 2), causal=False),
        c("dh128_L272", "train", (1, 272, 256, 2)),
        c("dh32_L496", "train", (1, 496, 64, 2)),
        c("dh32_L257_leftpad", "train", (3, 257, 64, 2), left_pad=True),
        c("dh32_L257_fixed", "general", (2, 257, 64, 2), combine="fixed"),
        c("dh32_L257_annealing_037", "general", (2, 257, 64, 2), combine="annealing", anneal_rate=0.37),
        c("dh32_L257_readrow", "train", (3, 257, 64, 2), pattern="calibrated_read_row"),
        c("dh32_L257_att_mask", "train", (3, 257, 64, 2), pattern="attacked_read_row_plus_mask"),
        c("dh32_L257_dense_plus_mask", "train", (2, 257, 64, 2), pattern="calibrated_dense_plus_mask"),
        c("dh32_L224_dense_LL", "general", (2, 224, 64, 2), mask="dense_LL"),
        c("dh32_L224_dense_L", "general", (2, 224, 64, 2), mask="dense_L", causal=False),
    ]


CASES = _table()
assert len({c.id for c in CASES}) == len(CASES)
