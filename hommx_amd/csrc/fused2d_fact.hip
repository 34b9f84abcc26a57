// fused2d_fact.hip -- the factor-emitting instantiations k_poisson2d_fused<NB, true, false> of fused2d.hip and their launch, as a translation unit
// of their own: in one module with <NB, false, false> they change the code the compiler generates for the tensor path (see the launch section
// of fused2d.hip).
#define HOMMX_FUSED_FACT_TU
#include "fused2d.hip"
