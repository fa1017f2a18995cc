// hsddp_phases.cpp — phase layouts and HKDProblem::update's bookkeeping on the host (hsddp_phases.h).
#include "hsddp_phases.h"

#include <cmath>
#include <cstring>

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

namespace {
// approx_eq_scalar / approx_leq_scalar / approx_geq_scalar (HSDDP_Utils.h:46-78)
bool approx_eq(float a, float b) { return std::abs(a - b) <= 1e-6f; }
bool approx_leq(float a, float b) { return a < b || approx_eq(a, b); }
bool approx_geq(float a, float b) { return a > b || approx_eq(a, b); }
}  // namespace

int segment_window(const hsddp_quad_state *w, int n_window, float dt_ref, float plan_duration, float dt_sim,
                   float dt_mpc, hsddp_phase_plan *plan, std::string &why)
{
    if (!w || !plan || n_window < 1) { why = "null argument / empty window"; return HSDDP_ERR_ARG; }
    if (!(dt_ref > 0) || !(dt_sim > 0)) { why = "dt_ref and dt_sim must be > 0"; return HSDDP_ERR_ARG; }
    const int sz = n_window - 1;
    std::memset(plan, 0, sizeof *plan);
    int prev[4], cur[4];
    double dur[4];
    auto contact = [&](int *c, float t) { std::memcpy(c, w[sample_at(t, dt_ref, sz)].contact, 4 * sizeof(int)); };
    auto duration = [&](double *d, float t) { std::memcpy(d, w[sample_at(t, dt_ref, sz)].status_dur, 4 * sizeof(double)); };
    float t = 0.0f, start = 0.0f;
    contact(prev, t);
    duration(dur, t);
    int P = 0;
    while (approx_leq(t, plan_duration)) {
        contact(cur, t);
        const bool change = std::memcmp(cur, prev, sizeof cur) != 0;
        if (change || approx_geq(t, plan_duration)) {
            if (P >= HSDDP_MAX_PHASES) { why = "more than HSDDP_MAX_PHASES phases"; return HSDDP_ERR_ARG; }
            const float end = t;
            plan->start_times[P] = start;
            plan->end_times[P] = end;
            plan->horizons[P] = (int)std::round((end - start) / dt_sim);
            std::memcpy(plan->contacts[P], prev, sizeof prev);
            std::memcpy(plan->durations[P], dur, sizeof dur);
            ++P;
            std::memcpy(prev, cur, sizeof cur);
            duration(dur, t);
            start = end;
        }
        t += dt_sim;
    }
    plan->n_phases = P;
    // the last phase's next contact (add_tconstr_one_phase, HKDProblem.cpp:272-276)
    contact(plan->contacts[P], plan_duration + dt_mpc);
    for (int i = 0; i < P; ++i)
        if (plan->horizons[i] < 1) { why = "a phase of zero knots (dt_sim too coarse)"; return HSDDP_ERR_ARG; }
    return HSDDP_OK;
}

int plan_restart(const hsddp_quad_state *table, int n_table, int start, int win_len, float dt_ref,
                 float plan_duration, float dt_sim, float dt_mpc, int Kc, RestartPlan &out, std::string &why)
{
    if (!table || start < 0 || start >= n_table) { why = "window start outside the table"; return HSDDP_ERR_ARG; }
    if (win_len < 1) { why = "empty reference window"; return HSDDP_ERR_ARG; }
    hsddp_phase_plan plan;
    const int n_window = win_len < n_table - start ? win_len : n_table - start;
    if (int rc = segment_window(table + start, n_window, dt_ref, plan_duration, dt_sim, dt_mpc, &plan, why)) return rc;
    if (plan.n_phases < 1) { why = "the window holds no phase"; return HSDDP_ERR_ARG; }
    out = RestartPlan{};
    if (int rc = build_layout(plan.n_phases, plan.horizons, nullptr, out.L, why)) return rc;
    if (control_slots(out.L) != Kc) { why = "the restarted window's horizons must sum to the handle's Kc"; return HSDDP_ERR_ARG; }
    for (int i = 0; i <= plan.n_phases; ++i)
        for (int l = 0; l < 4; ++l) out.contacts[i * 4 + l] = plan.contacts[i][l];
    for (int i = 0; i < plan.n_phases; ++i)
        for (int l = 0; l < 4; ++l) out.durations[i * 4 + l] = plan.durations[i][l];
    return HSDDP_OK;
}

}  // namespace hsddp
