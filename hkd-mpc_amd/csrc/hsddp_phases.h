// hsddp_phases.h — the phase bookkeeping of the batched HS-DDP solver on the host: the layout of
// one element's phases, HKDProblem::update's edits of it (HKDProblem.cpp:117-222),
// HKDProblem::initialization's segmentation of a reference window (:15-68; hsddp_plan_phases and
// the restart of single elements, hsddp_restart_elements) and QuadReference's sample rounding.  No
// HIP header, no handle and no global state: a plain C++ compiler builds hsddp_phases.cpp on its
// own (tests/drivers/phases_check.cpp, restart_check.cpp).
#pragma once

#include <string>
#include <vector>

struct hsddp_quad_state;
struct hsddp_phase_plan;

namespace hsddp {

constexpr int MAXP = 16;  // HSDDP_MAX_PHASES (include/hsddp.h)

// Phase layout of one element: P phases of N_i knots, state slots s0_i .. s0_i + N_i, control slots
// k0_i .. k0_i + N_i - 1, shooting states ss_i; S = sum(N_i + 1).  Per-element layouts
// (hsddp_set_element_layouts) all have the handle's Kc.
struct Layout {
    int P, S, has_tail, pad;
    int N[MAXP], s0[MAXP], k0[MAXP], ss[MAXP];
};
static_assert(sizeof(Layout) == (4 + 4 * MAXP) * sizeof(int), "Layout goes to the device as it stands (Bufs::lay)");

// The layout of n_phases phases with the given horizons and shooting states (null: every knot a
// shooting state, N_i + 1).  Refused (a code of include/hsddp.h and its text in `why`): n_phases
// outside 1..16, a horizon < 1, ss_i outside 0 .. N_i + 1, non-shooting states anywhere but in the
// last phase (the knot-parallel rollout simulates them after the shooting ones, and only there).
// The control slots (the sum of the horizons) and S against a handle are the caller's to check.
int build_layout(int n_phases, const int *horizons, const int *shooting, Layout &L, std::string &why);
inline int control_slots(const Layout &L) { return L.k0[L.P - 1] + L.N[L.P - 1]; }

// one phase of a layout being shifted; slot labels name where each value comes from:
// state  >= 0: old Xbar slot, -1: zero, <= -2: old (working) X slot -2 - label;
// control >= 0: old control slot (Ubar and K), -1: zero
struct ShiftPhase {
    int N, ss, reach;
    std::vector<int> xs, us;
    int src = -1;         // the old phase it continues (-1: added by this shift)
    int add = 0;          // touchdown constraints appended by this shift (add_tconstr_one_phase)
    std::vector<int> rs;  // per control slot: the old slot its ReB parameters come from (-1: initial)
    int born = -1;        // src < 0: the step that started it
};

// HKDProblem::update's phase bookkeeping (HKDProblem.cpp:117-222) of one layout, one simulation
// step at a time: drop_front, then extend_back with the step's contact-change flag (a caller that
// reads the flag off the phases — hsddp_advance compares the new contact with the last phase's —
// looks at `ph` in between), and finish after the last step.  A refusal returns its code with the
// text in `why`, named after the entry point `who` ("shift", "advance").
struct PhaseStepper {
    std::vector<ShiftPhase> ph;
    int step = 0;  // steps completed

    PhaseStepper(const Layout &L, const int *reach);
    int drop_front(const char *who, std::string &why);
    int extend_back(int change, const char *who, std::string &why);
    // update_SS_config (HKDProblem.cpp:203-217), and the layout of the phases as they stand
    int finish(Layout &L, std::string &why);
};

// HKDProblem::initialization's segmentation (HKDProblem.cpp:15-68) of a window of n_window
// samples into `plan` (hsddp_plan_phases, include/hsddp.h), with the reference's float clock.
// A refusal returns its code with the text in `why`.
int segment_window(const hsddp_quad_state *w, int n_window, float dt_ref, float plan_duration, float dt_sim,
                   float dt_mpc, hsddp_phase_plan *plan, std::string &why);

// One element's problem started again (hsddp_restart_elements): the segmentation of the window of
// win_len samples at table[start] (clipped at the table's end), as a layout whose every state is a
// shooting state (update_SS_config(N + 1), HKDProblem.cpp:104), its contact rows 0 .. P (row P:
// the contact at plan_duration + dt_mpc) and its phases' contact durations.  No phase has reached
// its end (quirk A15) and the element's clock restarts at 0.  Refused: a start outside the table,
// and a plan whose horizons do not sum to the handle's Kc control slots.
struct RestartPlan {
    Layout L;
    int contacts[(MAXP + 1) * 4];
    double durations[MAXP * 4];
};
int plan_restart(const hsddp_quad_state *table, int n_table, int start, int win_len, float dt_ref,
                 float plan_duration, float dt_sim, float dt_mpc, int Kc, RestartPlan &out, std::string &why);

// sample index of relative time t in a window of sz + 1 samples (QuadReference.cpp:64-75, 81-91):
// left-clipped, moved right when past the half step, clamped to the window end
int sample_at(float t, float dt, int sz);

}  // namespace hsddp
