// mir_step_packed.hip -- the kinds of the contact-rich steps (step_packed, mir_step.h) of mir_step.hip: the same source, compiled
// with the SLP vectoriser on (Makefile: STEP16PACKED; the launcher in mir_step.hip says which object holds which kind).
#define MIR_STEP_PACKED_TU
#include "mir_step.hip"
