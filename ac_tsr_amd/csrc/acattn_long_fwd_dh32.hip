// Long-sequence forward (acattn_long_fwd.inc), head size 32.
#define ACATTN_LONG_DH 32
#include "acattn_long_fwd.inc"
