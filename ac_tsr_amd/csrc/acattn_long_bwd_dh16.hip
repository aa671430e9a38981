// Long-sequence backward (acattn_long_bwd.inc), head size 16.
#define ACATTN_LONG_DH 16
#include "acattn_long_bwd.inc"
