// Long-sequence backward (acattn_long_bwd.inc), head size 128.
#define ACATTN_LONG_DH 128
#include "acattn_long_bwd.inc"
