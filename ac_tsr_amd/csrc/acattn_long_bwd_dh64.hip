// Long-sequence backward (acattn_long_bwd.inc), head size 64.
#define ACATTN_LONG_DH 64
#include "acattn_long_bwd.inc"
