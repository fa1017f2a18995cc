// hsddp_measure.hip — the initial state formed from the robots' measured states (hsddp_hkd_state,
// hsddp_update_problem_measured).
//
// The first step of HKDMPCSolver::update (HKDMPC.cpp:118-129) with compute_hkd_state
// (HKD-TrajOpt/HKDModel.h:65-96): xinit = [eul, pos, omega, vel, qdummy] from the state fields of
// hkd_data_lcmt, where the qdummy of a leg in stance in the first phase is its foot position and of
// a swing leg its joint angles.
#include "hsddp_measure.h"

namespace hsddp {

// One thread per (robot, leg); the leg-0 thread also writes the 12 body entries.  The float fields
// widen exactly.  hkd_foot_position is called as k_model_foot calls it (a runtime leg index, one
// evaluation per thread), so both round alike (tests/test_gpu_measured.py compares them bit for bit).
__global__ __launch_bounds__(256) void k_hkd_state(const hsddp_robot_state *states, const int *contact,
                                                   int contact_stride, double *x, int n)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= 4L * n) return;
    const size_t b = (size_t)(gid >> 2);
    const int l = (int)(gid & 3);
    const hsddp_robot_state &m = states[b];
    double *xo = x + b * NX;
    const double eul[3] = {(double)m.rpy[2], (double)m.rpy[1], (double)m.rpy[0]};
    const double pos[3] = {(double)m.p[0], (double)m.p[1], (double)m.p[2]};
    const double q[3] = {(double)m.qJ[3 * l], (double)m.qJ[3 * l + 1], (double)m.qJ[3 * l + 2]};
    if (l == 0) {
        for (int a = 0; a < 3; ++a) {
            xo[a] = eul[a];
            xo[3 + a] = pos[a];
            xo[6 + a] = (double)m.omegaBody[a];
            xo[9 + a] = (double)m.vWorld[a];
        }
    }
    double qd[3] = {q[0], q[1], q[2]};
    if (contact[b * (size_t)contact_stride + l] != 0) hkd::hkd_foot_position(l, pos, eul, q, qd);
    for (int a = 0; a < 3; ++a) xo[12 + 3 * l + a] = qd[a];
}

void launch_hkd_state(const hsddp_robot_state *states, const int *contact, int contact_stride, double *x, int n,
                      hipStream_t st)
{
    const long threads = 4L * n;
    hipLaunchKernelGGL(k_hkd_state, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, states, contact,
                       contact_stride, x, n);
}

}  // namespace hsddp
