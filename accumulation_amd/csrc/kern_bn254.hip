// Elliptic-curve kernels instantiated for BN254 G1 (254-bit base field, 8 x u32 limbs in memory, 9 x 29 bits in registers).
#include "kern_ec.inc"
AMSM_EC_LAUNCHERS(Bn254Fq)
