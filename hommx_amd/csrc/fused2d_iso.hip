// fused2d_iso.hip -- the unstratified instantiations k_poisson2d_fused<NB, false, true> of fused2d.hip and their launch, as a translation
// unit of their own: instantiations in one module change each other's schedule (see the launch section of fused2d.hip).
#define HOMMX_FUSED_ISO_TU
#include "fused2d.hip"
