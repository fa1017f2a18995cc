// hsddp_phases.cpp — phase layouts and HKDProblem::update's bookkeeping on the host (hsddp_phases.h).
#include "hsddp_phases.h"

#include <cmath>

#include "../../include/hsddp.h"

namespace hsddp {

static_assert(MAXP == HSDDP_MAX_PHASES, "phase capacity");

int build_layout(int n_phases, const int *horizons, const int *shooting, Layout &L, std::string &why)
{
    L = Layout{};
    if (n_phases < 1 || n_phases > MAXP) { why = "n_phases must lie in 1..16"; return HSDDP_ERR_ARG; }
    L.P = n_phases;
    int s = 0, k = 0;
    for (int i = 0; i < n_phases; ++i) {
        const int N = horizons[i], ss = shooting ? shooting[i] : N + 1;
        if (N < 1) { why = "phase horizons must be >= 1"; return HSDDP_ERR_ARG; }
        if (ss < 0 || ss > N + 1) { why = "shooting states must lie in 0 .. N_i + 1"; return HSDDP_ERR_ARG; }
        if (ss < N + 1 && i < n_phases - 1) { why = "non-shooting states outside the last phase"; return HSDDP_ERR_UNSUPPORTED; }
        L.N[i] = N; L.s0[i] = s; L.k0[i] = k; L.ss[i] = ss;
        L.has_tail |= ss < N + 1;
        s += N + 1; k += N;
    }
    L.S = s;
    return HSDDP_OK;
}

PhaseStepper::PhaseStepper(const Layout &L, const int *reach) : ph(L.P)
{
    for (int i = 0; i < L.P; ++i) {
        ph[i].N = L.N[i]; ph[i].ss = L.ss[i]; ph[i].reach = reach[i];
        ph[i].src = i;
        for (int k = 0; k <= L.N[i]; ++k) ph[i].xs.push_back(L.s0[i] + k);
        for (int k = 0; k < L.N[i]; ++k) ph[i].us.push_back(L.k0[i] + k);
        ph[i].rs = ph[i].us;
    }
}

// front: a first phase of one knot shrinks to a point and is removed (pop_front_phase,
// HKDProblem.h:56-66); otherwise its first knot is dropped (SinglePhase::pop_front,
// SinglePhase.cpp:496-501)
int PhaseStepper::drop_front(const char *who, std::string &why)
{
    if (ph.front().N <= 1) {
        if (ph.size() == 1) { why = std::string(who) + " would remove the only phase"; return HSDDP_ERR_ARG; }
        ph.erase(ph.begin());
    } else {
        ShiftPhase &f = ph.front();
        f.xs.erase(f.xs.begin());
        f.us.erase(f.us.begin());
        f.rs.erase(f.rs.begin());
        f.N--;
    }
    return HSDDP_OK;
}

// back: a contact change after the last phase reached its end starts a new phase of one knot with
// a zero trajectory (Trajectory::create_data); otherwise the last phase grows by
// push_back_default: X.back() copied into X and Xbar, zero control and gain (SinglePhase.cpp:
// 485-490, TrajectoryManagement.cpp:163-190)
int PhaseStepper::extend_back(int change, const char *who, std::string &why)
{
    ShiftPhase &l = ph.back();
    if (change && l.reach) {
        if ((int)ph.size() >= HSDDP_MAX_PHASES) { why = std::string(who) + " exceeds HSDDP_MAX_PHASES phases"; return HSDDP_ERR_ARG; }
        ShiftPhase n;
        n.N = 1; n.ss = 0; n.reach = 0;
        n.xs = {-1, -1};
        n.us = {-1};
        n.rs = {-1};  // a new GRF constraint: initial ReB parameters (HKDProblem.cpp:255-263)
        n.born = step;
        ph.push_back(n);
    } else {
        const int last = l.xs.back();
        l.xs.push_back(last >= 0 ? -2 - last : last);
        l.us.push_back(-1);
        l.rs.push_back(l.rs.back());  // PathConstraintBase::push_back copies params.back()
        l.N++;
        if (change) l.reach = 1;
    }
    // add_tconstr_one_phase on a last phase that has reached its end, at every step
    // (HKDProblem.cpp:199-202): one more touchdown constraint with initial AL parameters
    if (ph.back().reach) ph.back().add++;
    ++step;
    return HSDDP_OK;
}

// every phase but a last one of horizon <= 2 gets all its states as shooting states
int PhaseStepper::finish(Layout &L, std::string &why)
{
    const int P = (int)ph.size();
    int hz[MAXP], ss[MAXP];
    for (int i = 0; i < P; ++i) {
        if (i < P - 1 || ph[i].N > 2) ph[i].ss = ph[i].N + 1;
        hz[i] = ph[i].N;
        ss[i] = ph[i].ss;
    }
    return build_layout(P, hz, ss, L, why);
}

int sample_at(float t, float dt, int sz)
{
    int k = (int)std::floor(t / dt);
    if (t - k * dt > 0.5 * dt) k++;
    return k > sz ? sz : k;
}

}  // namespace hsddp
