// Elliptic-curve kernels instantiated for Vesta (255-bit base field = Pallas's scalar field, 8 x u32 limbs).
#define AMSM_FQ VestaFq
#define AMSM_FR VestaFr  // the curve's scalar field (GLV split of fold scalars, host_glv.h)
#define AMSM_CURVE_ID 2
#include "kern_ec.inc"
