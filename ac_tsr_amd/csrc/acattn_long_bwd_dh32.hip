// Long-sequence backward (acattn_long_bwd.inc), head size 32.
#define ACATTN_LONG_DH 32
#include "acattn_long_bwd.inc"
