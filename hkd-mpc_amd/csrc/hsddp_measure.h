// hsddp_measure.h — kernel interface of the measured-state ingest (hsddp_measure.hip).
#pragma once

#include "../../include/hsddp.h"
#include "hsddp_internal.h"

namespace hsddp {

// x[n][24] from states[n]; robot b's contact row is contact[b * contact_stride .. + 3] (4 for the
// model primitive's [n][4] rows, (P + 1) * 4 for row 0 of a handle's contacts)
void launch_hkd_state(const hsddp_robot_state *states, const int *contact, int contact_stride, double *x, int n,
                      hipStream_t st);

}  // namespace hsddp
