// hsddp_phases.h — the bookkeeping of the batched HS-DDP solver on the host: the layout of one
// element's phases, HKDProblem::update's edits of it (HKDProblem.cpp:117-222),
// HKDProblem::initialization's segmentation of a reference window (:15-68; hsddp_plan_phases),
// QuadReference's sample rounding, and on top of them the plans of the MPC caller's entry points:
// the shift's slot maps, hsddp_advance's walk over the reference table, the references' slot
// samples, hsddp_restart_elements' and hsddp_copy_elements' batch decisions and the sweep's pairing
// of equal layouts.  The entry points (hsddp_horizon.cpp, hsddp_api.cpp) check, call a plan here,
// apply it on the device and commit it to the handle.  No HIP header, no handle and no global state: the handle's host
// fields are read through a HorizonView, and a plain C++ compiler builds hsddp_phases.cpp on its
// own (tests/drivers/phases_check.cpp, restart_check.cpp, horizon_check.cpp, elements_check.cpp).
#pragma once

#include <cstddef>
#include <map>
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

// ---- elements grouped by an integer key ---------------------------------------------------------
// key -> index in order of first sight.  A caller that builds something per new key compares the
// index with size() taken before the call.
struct Interner {
    std::map<std::vector<int>, int> ids;
    int size() const { return (int)ids.size(); }
    int operator()(std::vector<int> key) { return ids.try_emplace(std::move(key), size()).first->second; }
};

// a layout's horizons, and with_ss: a -1 and its shooting states (two layouts of equal key are equal)
std::vector<int> layout_key(const Layout &L, bool with_ss);
// the key under which elements share a slot map: layout, reach flags, step flags
std::vector<int> shift_key(const Layout &L, const int *reach, int n_steps, const int *cc);

// ---- the handle's host state, read-only (hsddp_handle.h: view_of) -----------------------------------
struct HorizonView {
    int B, Bref, Kc;
    int P, S;               // strides of the per-phase and per-slot rows (the batch's largest layout)
    size_t S_cap;
    const Layout *shared;   // the batch's layout, or
    const Layout *lays;     // [B] per-element layouts (null: shared)
    const int *reach;       // is_phase_reach_end: [P] shared, [B][MAXP] per element
    const int *contacts;    // [B][P + 1][4]
    const double *durations;  // [B][P][4]
    const hsddp_quad_state *table;  // [ref_n] samples dt_ref apart
    int ref_n;
    float ref_dt;
    const int *win_start;   // [Bref]
    int win_len;
    float dt_sim;
    float t_cur;            // QuadReference::t_cur of the batch, or
    const float *t_el;      // [B] each element's own (null: t_cur)
    const double *terrain;  // [B][P][2] (mu, ground) per phase (hsddp_set_terrain), or null: off
    double fill[2];         // the handle's cparams pair: the row of a phase without one of its own
    const double *weights;  // [B][NW] per-robot weight rows (hsddp_set_element_weights), or null: off
    const int *pw_set;      // [B][P] a phase's weights are an override (hsddp_set_phase_weights), or null: none
    const double *pw;       // [B][P][NW] the override rows (read where pw_set is set)

    const Layout &layout(int b) const { return lays ? lays[b] : *shared; }
    const int *reach_of(int b) const { return lays ? reach + (size_t)b * MAXP : reach; }
};

// ---- the shift ----------------------------------------------------------------------------------
// the bookkeeping's outcome: per slot map the phases after the steps (PhaseStepper) and their
// layout, and the map of each element (elements with equal layout, reach flags and step flags
// share one)
struct ShiftPlan {
    std::vector<std::vector<ShiftPhase>> phs;
    std::vector<Layout> nl;
    std::vector<int> map_id;  // [B]
    // is_phase_reach_end of map q's phases
    void reach(int q, int *out) const { for (size_t i = 0; i < phs[q].size(); ++i) out[i] = phs[q][i].reach; }
};

// hsddp_shift / hsddp_shift_elements: every element shifted by the caller's flags,
// cc[b * bstride + j] element b's flag of step j (bstride 0: one set for the batch).  Refused:
// what PhaseStepper refuses, and shifts that diverge under shared references.
int plan_shift(const HorizonView &v, int n_steps, const int *cc, size_t bstride, ShiftPlan &plan, std::string &why);

// A plan as the gather kernels read it: slot maps [nk][S_new] (padding rows -1: zero) and
// [nk][Kc], the ReB source per control slot [nk][Kc], the phase source and appended touchdown
// constraints [nk][MAXP].  Refused: a layout past the handle's Kc or S_cap.
struct ShiftMaps {
    int S_new = 0, P_new = 0;
    std::vector<int> smap, cmap, rmap, pmap, nadd;
};
int flatten_shift(const ShiftPlan &plan, int Kc, size_t S_cap, ShiftMaps &m, std::string &why);
// the elements' layouts and reach flags [B][MAXP] after a plan of several maps
void shifted_layouts(const ShiftPlan &plan, std::vector<Layout> &lays, std::vector<int> &reach);

// ---- terrain ---------------------------------------------------------------------------------------
// The per-phase (mu, ground) rows move with the phases as the contact durations do.  The view's
// rows after a shift plan, [B][P][2] at the new stride P: an old phase keeps its row, a phase the
// steps started takes the row of the phase before it (the element's previous last phase); the rows
// past an element's phases, and an element whose first phase is new (its rows are a restart's or an
// arriving element's to write), hold the view's fill.  (Reads the view's terrain and fill only.)
void shift_terrain(const HorizonView &v, const ShiftPlan &plan, int P, std::vector<double> &out);
// one element's rows at stride P: its own n rows (null: fill), fill past them
void put_terrain_rows(const double *rows, int n, int P, const double *fill, double *out);

// ---- per-phase weights ------------------------------------------------------------------------------
// An override (hsddp_set_phase_weights) belongs to its phase's cost objects.  The view's flags [B][P]
// and rows [B][P][NW] after a shift plan, at the new stride P: an old phase keeps its flag and row;
// a phase the steps started has none (create_problem_one_phase constructs new cost objects — where
// the terrain row of a new phase repeats the one before it), nor has a phase without a source or one
// past an element's phases.  Rows without a flag are zero.  (Reads the view's pw_set and pw only.)
void shift_phase_weights(const HorizonView &v, const ShiftPlan &plan, int P, std::vector<int> &set, std::vector<double> &rows);
// one element's flags and rows at stride P: its own n (null: none), none past them
void put_phase_weight_rows(const int *set, const double *rows, int n, int P, int *out_set, double *out_rows);

// ---- references ------------------------------------------------------------------------------------
// the phases' start times on the float clock of HKDProblem::initialization (t += dt_sim per knot)
std::vector<float> clock_starts(const Layout &L, float dt_sim);
// the window sample of every state slot of layout L, S entries (padding slots repeat the last
// sample): slot times as the reference forms them, t_offset (float, phase start relative to the
// first phase) + k dt (double), passed on as float (SinglePhase.cpp:243-287; set_time_offset,
// HKDProblem.cpp:103,208), snapped to a sample (QuadReference.cpp:60-76)
std::vector<int> slot_samples(const Layout &L, const std::vector<float> &start, float dt_sim, float dt_ref, int sz, int S);

// one slot map per distinct layout: idx [n_maps][S]; add returns the layout's map.  The phases
// start at phase_start_times (relative to the first), or on the float clock (null).
struct SlotMaps {
    Interner keys;
    std::vector<int> idx;
    std::vector<std::vector<float>> starts;  // per map
    int add(const Layout &L, const float *phase_start_times, float dt_sim, float dt_ref, int sz, int S);
};

// hsddp_build_references' host side: the slot maps of the view's layouts (map_id [B] with
// per-element layouts, else empty), and for a new problem the contact duration of every phase
// [B][P][4], read at its start time as HKDProblem::initialization does
// (get_contact_duration_at_t at t = 0 and at each phase end, HKDProblem.cpp:38,63)
struct RefPlan {
    std::vector<int> idx, map_id;
    std::vector<double> durations;
};
void plan_refs(const HorizonView &v, const int *window_start, int window_len, const float *phase_start_times,
               float dt_sim, bool initial, RefPlan &out);

// ---- hsddp_advance ---------------------------------------------------------------------------------
// HKDProblem::update's bookkeeping (HKDProblem.cpp:126-202) of every element over n_steps
// simulation steps, the contacts read from the table: per step the window advances
// (QuadReference::step, QuadReference.cpp:33-47) and the contact at the new horizon end against
// the last phase's is the step's flag (PhaseStepper).  With the shared layout and window, an
// element whose contact rows equal element 0's steps as element 0 does: rep[b] = 0.
struct AdvanceWalk {
    struct Element {
        std::vector<int> flags;            // per step
        int P_old = 0;                     // phases before the steps
        int next_kind = 0, next_step = -1; // row P: 0 old row, 1 contact at rel, 2 at plan + dt_mpc
        int map = 0;
    };
    std::vector<Element> el;               // [B], filled where rep[b] == b
    std::vector<int> rep;                  // [B]
    std::vector<std::vector<int>> wsj;     // window starts [Bref] at each step
    std::vector<std::vector<float>> relj;  // new_end - new_start at each step, per clock
    std::vector<int> ws;                   // window starts after the steps
    std::vector<float> t_cur;              // clocks after the steps: one, or [B]
    ShiftPlan plan;
    bool agree = false;                    // one slot map and the shared layout stays shared
    std::vector<int> flags;                // per step: some element saw a contact change
};
// Refused: a window that runs past the table, what PhaseStepper refuses, and elements that
// disagree under shared references.
int walk_advance(const HorizonView &v, int n_steps, float plan_duration, AdvanceWalk &w, std::string &why);
// The contact rows [B][P + 1][4] and durations [B][P][4] after the walk, at the new stride P: an old
// phase keeps its row of the view's, a phase the steps started has the table's sample at the
// horizon end of its first step.  (Reads the view's contacts, durations, table and window only:
// the view may be the one the walk had, taken before the shift changed the handle's layouts.)
void advance_rows(const HorizonView &v, const AdvanceWalk &w, int P, float plan_duration, float dt_mpc,
                  std::vector<int> &contacts, std::vector<double> &durations);

// ---- hsddp_restart_elements ------------------------------------------------------------------------
std::vector<int> listed_elements(const int *mask, int B);

// The batch's side of a restart of the listed elements at window_start[b] (full [B] array): each
// one's RestartPlan, and what follows for the handle.
struct RestartBatch {
    std::vector<RestartPlan> plans;  // [n]
    bool all = false;       // every element restarts
    int Pn = 0, Sn = 0;     // the strides after the restart
    bool one = false;       // one layout for the batch stays (or becomes) the shared one
    bool restride = false;  // a stride changes: every element's rows move
    bool in_place = false;  // per-element layouts and the strides stand: only the listed rows change
    std::vector<Layout> lays;  // none of the three: every element's layout and reach flags
    std::vector<int> reach;
    ShiftPlan stride_plan;  // restride: a shift of no steps (identity maps; the listed elements' rows zero)
    std::vector<int> contacts;  // restride: [B][Pn + 1][4] and [B][Pn][4], the listed elements' new rows in
    std::vector<double> durations;
    std::vector<int> rows;  // the listed elements' contact rows, compacted [n][Pn + 1][4]
    SlotMaps slots;         // one per distinct new layout, Sn wide
    std::vector<int> map_id, start;  // [n] each listed element's slot map and window start
    std::vector<int> win_start;      // [Bref] after the restart
    std::vector<float> t_el;         // the clocks after the restart (empty: shared, at t_cur)
    float t_cur = 0;                 // the batch's shared clock after it (a restart of every element: 0)
    std::vector<int> reach_in;       // [n][MAXP] the listed elements' reach flags (a restart: none)
};
// Refused: differing window starts under shared references, what plan_restart refuses, S past S_cap.
int plan_restart_batch(const HorizonView &v, const std::vector<int> &list, const int *window_start,
                       float plan_duration, float dt_mpc, RestartBatch &r, std::string &why);
// one listed element's new rows at stride P: contacts [P + 1][4] and durations [P][4], zero past its phases
void put_restart_rows(const RestartPlan &plan, int P, int *contacts, double *durations);

// ---- hsddp_copy_elements / hsddp_import_elements ---------------------------------------------------
// What the host holds of one element between ticks, as an element record carries it: layout, reach
// flags, contact rows 0 .. P, contact durations (zero without a reference table), window start and
// QuadReference clock.  Rows past the element's phases are zero.
constexpr int NW = 46;  // doubles of one hsddp_hkd_weights (include/hsddp.h)
struct ElementImport {
    Layout L;
    int reach[MAXP];
    int contacts[(MAXP + 1) * 4];
    double durations[MAXP * 4];
    int win_start;
    float clock;
    int has_terrain;              // the source's terrain was on: terrain holds the element's rows
    double terrain[MAXP * 2];     // (mu, ground) per phase
    int has_weights;              // the source's weight table was on: weights holds the robot's row
    double weights[NW];           // (the fields of hsddp_hkd_weights, in order)
};
// ... and its phase overrides (hsddp_set_phase_weights), carried beside it: a record holds them in a
// block of its own between the header and the payload (hsddp_elements.h)
struct PhaseOverrides {
    int has;                      // the element has overrides: set flags them, rows holds their rows
    int set[MAXP];
    double rows[MAXP * NW];       // (zero where set is 0)
};
// element b of the view
void export_element(const HorizonView &v, int b, ElementImport &out);
void export_overrides(const HorizonView &v, int b, PhaseOverrides &out);
// The batch's side of slot list[m] becoming the element in[m]: plan_restart_batch's decisions (one,
// restride, in_place, strides, contact and duration rows, window starts; patch_pairs follows as
// there) with each listed element's layout, reach flags, rows, window start and clock taken from
// in[m] instead of a segmentation.  No slot maps (the reference rows arrive with the element).  The
// batch keeps one clock while every element's equals it, else it moves to per-element clocks.
// Refused: an index outside the batch or named twice, a layout that is not one of Kc control slots,
// S past S_cap.
int plan_import_batch(const HorizonView &v, const std::vector<int> &list, const ElementImport *in, RestartBatch &r,
                      std::string &why);

// ---- sweep pairs -----------------------------------------------------------------------------------
// Two elements of equal layout (layout_key with ss) per wave: pairs [n_pairs][2], -1 for no partner,
// groups in key order and elements in index order within a group.
std::vector<int> pair_layouts(const std::vector<Layout> &lays);
// The pairs after the listed elements took new layouts (lays holds them already), patched in place:
// a listed element leaves its pair (its partner stays alone), the listed elements pair up among
// themselves by new layout, emptied entries are filled from the end.  Returns the entries written
// (those >= n_pairs are gone).
std::vector<int> patch_pairs(std::vector<int> &pairs, std::vector<int> &pair_of, int &n_pairs, const Layout *lays,
                             const std::vector<int> &list);

}  // namespace hsddp
