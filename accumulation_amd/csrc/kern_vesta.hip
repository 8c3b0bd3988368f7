// Elliptic-curve kernels instantiated for Vesta (255-bit base field = Pallas's scalar field, 8 x u32 limbs).
#include "kern_ec.inc"
AMSM_EC_LAUNCHERS(VestaFq)
