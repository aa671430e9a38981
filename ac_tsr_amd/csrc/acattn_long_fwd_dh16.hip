// Long-sequence forward (acattn_long_fwd.inc), head size 16.
#define ACATTN_LONG_DH 16
#include "acattn_long_fwd.inc"
