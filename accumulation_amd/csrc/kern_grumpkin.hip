// Elliptic-curve kernels instantiated for Grumpkin (254-bit base field, 8 x u32 limbs in memory, 9 x 29 bits in registers).
#define AMSM_FQ GrumpkinFq
#define AMSM_FR GrumpkinFr  // the curve's scalar field (GLV split of fold scalars, host_glv.h)
#define AMSM_CURVE_ID 6
#include "kern_ec.inc"
