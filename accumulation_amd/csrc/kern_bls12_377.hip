// Elliptic-curve kernels instantiated for BLS12-377 G1 (377-bit base field, 12 x u32 limbs in memory, 14 x 28 bits in registers).
#define AMSM_FQ Bls12377Fq
#define AMSM_FR Bls12377Fr  // the curve's scalar field (GLV split of fold scalars, host_glv.h)
#define AMSM_CURVE_ID 8
#include "kern_ec.inc"
