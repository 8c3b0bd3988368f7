// Elliptic-curve kernels instantiated for BLS12-377 G1 (377-bit base field, 12 x u32 limbs in memory, 14 x 28 bits in registers).
#include "kern_ec.inc"
AMSM_EC_LAUNCHERS(Bls12377Fq)
