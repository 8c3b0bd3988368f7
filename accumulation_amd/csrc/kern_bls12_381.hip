// Elliptic-curve kernels instantiated for BLS12-381 G1 (381-bit base field, 12 x u32 limbs).
#include "kern_ec.inc"
AMSM_EC_LAUNCHERS(Bls12381Fq)
