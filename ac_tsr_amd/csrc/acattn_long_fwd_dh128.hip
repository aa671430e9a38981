// Long-sequence forward (acattn_long_fwd.inc), head size 128.
#define ACATTN_LONG_DH 128
#include "acattn_long_fwd.inc"
