// Elliptic-curve kernels instantiated for Pallas (255-bit base field, 8 x u32 limbs).
#include "kern_ec.inc"
AMSM_EC_LAUNCHERS(PallasFq)
