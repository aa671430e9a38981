// Long-sequence forward (acattn_long_fwd.inc), head size 64.
#define ACATTN_LONG_DH 64
#include "acattn_long_fwd.inc"
