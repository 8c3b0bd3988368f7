// Elliptic-curve kernels instantiated for BN254 G1 (254-bit base field, 8 x u32 limbs in memory, 9 x 29 bits in registers).
#define AMSM_FQ Bn254Fq
#define AMSM_FR Bn254Fr  // the curve's scalar field (GLV split of fold scalars, host_glv.h)
#define AMSM_CURVE_ID 4
#include "kern_ec.inc"
