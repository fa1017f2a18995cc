// hsddp_simulate.h — kernel interface of the policy simulation (hsddp_simulate.hip).
#pragma once

#include "../../include/hsddp.h"
#include "hsddp_internal.h"

namespace hsddp {

// hsddp_simulate_policy's device arguments: M samples of n_steps knots per element
struct SimArgs {
    int M, n_steps;
    const double *x_init;       // [B][M][24], or null: every sample starts at Bufs::x0[b]
    double *x_end;              // [B][M][24]
    hsddp_sim_sample *summary;  // [B][M], or null
    double *X, *U;              // [B][M][n_steps][24] zeroed by the caller, or null
};
// terrain: the per-phase (mu, ground) pairs min_grf / max_td are taken against, or null (hsddp_internal.h)
void launch_simulate_policy(const Params &p, const Bufs &d, const SimArgs &a, const double *terrain, WtsTab weights,
                            hipStream_t st);

}  // namespace hsddp
