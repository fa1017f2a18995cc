// hsddp_handle.h — the handle behind include/hsddp.h and the host helpers its source files share
// (private to csrc): hsddp_api.cpp (handle, layouts, transfers), hsddp_solve.cpp (the solve loop),
// hsddp_horizon.cpp (the MPC caller's side: commands, shift, references, hsddp_advance, restarts)
// and hsddp_settings.cpp (defaults and the INFO loaders).  The host bookkeeping those entry points
// plan with is hsddp_phases.cpp, which sees the handle's host fields through view_of() only.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hsddp.h"
#include "hsddp_internal.h"

namespace hsddp {
// records the calling thread's hsddp_last_error text; returns code (hsddp_api.cpp)
int fail(int code, const std::string &msg);
}  // namespace hsddp

#define HIPCHK(expr)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return hsddp::fail(HSDDP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct hsddp_handle_t {
    using Params = hsddp::Params;
    using Bufs = hsddp::Bufs;
    using Layout = hsddp::Layout;
    // the slot costs / |Defect|^2 of the last rollout (k_rollout's per-slot outputs) belong to the
    // working trajectory under the current cost parameters: k_lq need not recompute them
    bool slots_fresh = false;
    // every per-knot ReB (delta, eps) still equals the descriptor's initial pair, so the kernels may
    // read the two scalars (Params::reb_uniform) when the schedule keeps them there
    bool reb_at_init = true;
    hsddp_problem_desc desc;
    hsddp_options opt;
    Params p;
    Bufs d;
    hipStream_t stream = nullptr;
    int *host_counter = nullptr;                // [16]: k_count's activity counts, stat sums, the graphs' counts
    std::vector<hipEvent_t> events;             // the stats timer's pool (reused, destroyed with the handle)
    // hsddp_solve's inner iteration + activity count as replayed hipGraphs (early-exit mode), keyed
    // by the launch arguments they froze; a small cache so the receding-horizon tick's recurring
    // layouts and swapped warm-start buffers find theirs again (round-robin eviction)
    struct IterGraph {
        hipGraphExec_t exec = nullptr;
        Params p;
        Bufs d;
        double alpha = 0;
        const int *budget = nullptr;
        const double *terrain = nullptr;
        const hsddp::Wts *weights = nullptr;
        const hsddp::PWts *phase_weights = nullptr;
        int par = 0;  // which host count slot (host_counter[8 + 4 * par + 1]) its copy fills
    } iter_graph[8];
    int iter_graph_next = 0;
    // hsddp_advance's shift without its own synchronisation: the host rows its pageable copies read
    // stay here until the advance synchronises, and the touchdown-overflow flag is read then
    std::vector<std::vector<int>> shift_keep;
    bool shift_overflow_pending = false;
    size_t scratch_reserved = 0;  // scratch bytes the pending shift's maps occupy (build_refs goes after)
    hipEvent_t iter_done[2] = {nullptr, nullptr};  // recorded after each replay, by parity
    std::vector<void *> allocs;
    size_t bytes = 0;
    int Bref = 1;
    bool have_problem = false;
    std::vector<int> contacts;  // host copy [B][P+1][4]: maps the compact K rows to controls
    bool contacts_current = false;  // `contacts` belong to the current layout (not stale after a shift)
    void *scratch = nullptr;    // device staging for the MPC-side calls (grown on demand)
    size_t scratch_bytes = 0;
    // receding-horizon state (HKDProblemData, HKDProblem.h:20-66): is_phase_reach_end per phase,
    // state-slot capacity (a shift keeps Kc and may add phases), and the second set of compact gain
    // rows the shift gathers into (allocated by the first shift; the new Xbar / Ubar rows go to each
    // element's third trajectory buffer)
    std::vector<int> reach_end;
    size_t S_cap = 0;
    void *spare_K = nullptr;
    // ... and of the constraint parameters the phases carry (ReB per knot, touchdown constraints)
    double *spare_reb_delta = nullptr, *spare_reb_eps = nullptr, *spare_al_sigma = nullptr, *spare_al_lambda = nullptr;
    int *spare_td_mask = nullptr;
    double *spare_cf_u = nullptr;
    int *spare_cf_flag = nullptr;
    double *shift_stage = nullptr;  // [3][B][S_cap][24] (ShiftArgs::stage), at the first stride-changing shift
    // ... and of the search direction (dX [B][S_cap][24]; dU, du [B][Kc][24]), which has one buffer each
    double *spare_dX = nullptr, *spare_dU = nullptr, *spare_du = nullptr;
    bool need_inputs = false;   // a shift changed the layout: update_problem before solving
    double *ref_table = nullptr;  // reference samples [n][RT_W] (hsddp_set_reference_table)
    int ref_n = 0;
    float ref_dt = 0;
    unsigned long long table_key = 0;  // hash of the table's samples (the element records' compatibility key)
    bool refs_on_device = false;  // references built by hsddp_build_references for this layout
    bool ref_cols_stale = true;   // Bufs::ref_t behind the reference rows (refreshed by begin_launches)
    // reference-driven MPC state (hsddp_advance): the table's samples on the host (contacts and
    // durations are read there), each reference element's window start, the window length and
    // the simulation step of the last hsddp_build_references, QuadReference::t_cur, and the
    // contact durations of every element's phases [B][P][4] (HKDProblemData::contact_durations)
    std::vector<hsddp_quad_state> table_host;
    std::vector<int> win_start;
    int win_len = 0;
    float dt_sim = 0, t_cur = 0;
    // each element's own clock [B] once hsddp_restart_elements has set some element's back to 0
    // (empty: the batch shares t_cur)
    std::vector<float> t_el;
    std::vector<double> durations;
    int retry_cap_alloc = 0, retry_m_alloc = 0;  // parallel regularisation retry scratch (k_riccati_retry)
    float *hist = nullptr;  // solver-info history [B][p.hcap][4] (grown by ensure_history)
    // per-element layouts (hsddp_set_element_layouts): host copies of Bufs::lay; empty = the handle's
    // shared one (adopt_shared_layout; Params carries its N / s0 / k0 / ss to the kernels)
    Layout shared{};
    std::vector<Layout> lays;
    std::vector<int> reach_el;  // [B][16] is_phase_reach_end per element (with per-element layouts)
    // host copy of Bufs::pairs [n_pairs][2] and each element's pair (set_layouts; patched in place by
    // hsddp_restart_elements)
    std::vector<int> pairs_host, pair_of;
    double *value0 = nullptr;  // G[0], H[0] per phase [B][16][600] (hsddp_set_value_export)
    // asynchronous command extraction (hsddp_extract_commands_async): two device record buffers, two
    // pinned host buffers, a copy stream and per buffer the event of its last copy
    hsddp_mpc_command *cmd_dev[2] = {nullptr, nullptr}, *cmd_host[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;
    hipEvent_t cmd_ready[2] = {nullptr, nullptr}, cmd_copied[2] = {nullptr, nullptr};
    char *cmd_in_host[2] = {nullptr, nullptr};  // pinned staging of each ticket's durations / feet
    size_t cmd_in_bytes[2] = {0, 0};
    int cmd_next = 0;
    // policy simulation (hsddp_simulate_policy): its device buffers (x_end first, then x_init, the
    // summaries and the optional X / U rows; grown on demand), and what hsddp_update_problem_simulated
    // checks: the samples and steps of the simulation held, whether the policy it ran is still the
    // handle's (no solve or warm-start upload since) and the steps shifted since
    char *sim_buf = nullptr;
    size_t sim_bytes = 0;
    int sim_M = 0, sim_n = 0, sim_shifted = 0;
    bool sim_fresh = false;
    // measured states (hsddp_update_problem_measured): the device copy of records that came from the
    // host [B], the handle's own copy of the records' foot placements [B][12] (both allocated on
    // first use), and whether that copy belongs to the current tick (an update with a host-formed or
    // simulated x0 drops it)
    // per-element iteration budgets (hsddp_set_element_budgets): the device array [B][2] (allocated
    // on first use), whether it is in force, the largest outer and inner bound (the host's loop
    // bounds) and the largest outer x inner product (the solver-info history's size)
    int *budgets = nullptr;
    bool budgets_on = false;
    int bud_AL = 0, bud_DDP = 0;
    long bud_hist = 0;
    hsddp_robot_state *meas_states = nullptr;
    float *meas_feet = nullptr;
    bool meas_held = false;
    // per-phase terrain (hsddp_set_terrain): the host rows [B][P][2] = (mu, ground) at the stride
    // p.P, rows past an element's phases at the cparams pair — the source of truth, moved with the
    // phases by hsddp_phases.cpp; empty: terrain off.  The device copy the terrain instantiations
    // read ([B][HSDDP_MAX_PHASES] pairs allocated on first use, so the pointer the iteration graphs
    // freeze never moves) is uploaded from pinned staging when the host rows changed (sync_terrain);
    // terrain_up: that upload's event (the staging is rewritten only after it)
    std::vector<double> terrain;
    double *terrain_dev = nullptr, *terrain_pin = nullptr;
    bool terrain_stale = false;
    hipEvent_t terrain_up = nullptr;
    // per-robot weights (hsddp_set_element_weights): the host rows [B] — the source of truth; they
    // belong to the robot, so shifts, advances and restarts leave them alone — empty: the table is
    // off and every robot has desc.weights.  The device copy the weights instantiations read ([B]
    // rows of Wts, allocated on first use, so the pointer the iteration graphs freeze never moves) is
    // uploaded from pinned staging when the host rows changed (sync_weights); weights_up: that
    // upload's event
    std::vector<hsddp_hkd_weights> weights;
    hsddp::Wts *weights_dev = nullptr, *weights_pin = nullptr;
    bool weights_stale = false;
    hipEvent_t weights_up = nullptr;
    // per-phase weights (hsddp_set_phase_weights): the override flags [B][P] and rows [B][P] at the
    // stride p.P — the source of truth, moved with the phases by hsddp_phases.cpp; both empty: no
    // phase has an override (they are emptied when the last one leaves).  The device copy the
    // per-phase instantiations read is the dense table of effective rows (override, else the robot's
    // row, else desc.weights), [B][HSDDP_MAX_PHASES] rows allocated on first use so the pointer the
    // iteration graphs freeze never moves, read at the stride p.P; it is uploaded from pinned staging
    // when an override, a flag, a robot's row beneath or the phase map changed (sync_phase_weights);
    // pw_up: that upload's event
    // (rows as doubles [B][P][NW], the form hsddp_phases.cpp moves them in: a shift's result is swapped in)
    std::vector<int> pw_set;
    std::vector<double> pw;
    hsddp::PWts *pw_dev = nullptr, *pw_pin = nullptr;
    bool pw_stale = false;
    hipEvent_t pw_up = nullptr;
};
static_assert(sizeof(hsddp_hkd_weights) == hsddp::NW * sizeof(double), "hsddp_hkd_weights: NW doubles, no padding");

namespace hsddp {

// device staging area of at least `bytes` (contents not preserved when it grows)
inline int scratch(hsddp_handle h, size_t bytes, char **out)
{
    if (bytes > h->scratch_bytes) {
        if (h->scratch) hipFree(h->scratch);
        h->scratch = nullptr;
        h->scratch_bytes = 0;
        hipError_t e = hipMalloc(&h->scratch, bytes);
        if (e != hipSuccess) return fail(HSDDP_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
        h->scratch_bytes = bytes;
    }
    *out = (char *)h->scratch;
    return HSDDP_OK;
}

// the layout of element b: the handle's, or its own (hsddp_set_element_layouts)
inline const Layout &layout_of(hsddp_handle h, size_t b)
{
    return h->lays.empty() ? h->shared : h->lays[b];
}

// is_phase_reach_end of element b's phases
inline const int *reach_of(hsddp_handle h, size_t b)
{
    return h->lays.empty() ? h->reach_end.data() : &h->reach_el[b * HSDDP_MAX_PHASES];
}

// the handle's host state as the bookkeeping reads it (hsddp_phases.h): pointers into the handle's
// own fields, good until a call changes them
inline HorizonView view_of(hsddp_handle h)
{
    HorizonView v{};
    v.B = h->p.B; v.Bref = h->Bref; v.Kc = h->p.Kc; v.P = h->p.P; v.S = h->p.S;
    v.S_cap = h->S_cap;
    v.shared = &h->shared;
    v.lays = h->lays.empty() ? nullptr : h->lays.data();
    v.reach = v.lays ? h->reach_el.data() : h->reach_end.data();
    v.contacts = h->contacts.data(); v.durations = h->durations.data();
    v.table = h->table_host.data(); v.ref_n = h->ref_n; v.ref_dt = h->ref_dt;
    v.win_start = h->win_start.data(); v.win_len = h->win_len; v.dt_sim = h->dt_sim;
    v.t_cur = h->t_cur;
    v.t_el = h->t_el.empty() ? nullptr : h->t_el.data();
    v.terrain = h->terrain.empty() ? nullptr : h->terrain.data();
    v.fill[0] = h->desc.cparams.mu_fric; v.fill[1] = h->desc.cparams.ground_height;
    v.weights = h->weights.empty() ? nullptr : (const double *)h->weights.data();
    v.pw_set = h->pw_set.empty() ? nullptr : h->pw_set.data();
    v.pw = h->pw_set.empty() ? nullptr : h->pw.data();
    return v;
}

// the budgets the kernels read (null: the handle-wide options) and the host's loop bounds
inline const int *budget_of(hsddp_handle h) { return h->budgets_on ? h->budgets : nullptr; }
inline int outer_bound(hsddp_handle h) { return h->budgets_on ? h->bud_AL : h->opt.max_AL_iter; }
inline int inner_bound(hsddp_handle h) { return h->budgets_on ? h->bud_DDP : h->opt.max_DDP_iter; }

// the table the kernels' terrain instantiations read (null: terrain off, the plain instantiations).
// Whoever turns terrain on allocates the table first (ensure_terrain_table), so host rows never go
// with a null table — which would launch the plain instantiations on a handle with terrain.
inline const double *terrain_of(hsddp_handle h) { return h->terrain.empty() ? nullptr : h->terrain_dev; }
// hsddp_api.cpp: the device table, its pinned staging and the upload's event (allocated once)
int ensure_terrain_table(hsddp_handle h);
// ... and the table brought up to the host rows on the handle's stream (before the launches of a
// call that reads it; never inside a graph capture)
int sync_terrain(hsddp_handle h);

// the weight table the kernels' weights instantiations read (null: off, the plain instantiations);
// whoever turns the table on allocates it first (ensure_weights_table), as with the terrain
// ... and the per-phase table of effective rows while a phase has an override
inline WtsTab weights_of(hsddp_handle h)
{
    return {h->weights.empty() ? nullptr : h->weights_dev, h->pw_set.empty() ? nullptr : h->pw_dev};
}
// robot b's weights: its row, or the handle's
inline const hsddp_hkd_weights &weights_of(hsddp_handle h, size_t b) { return h->weights.empty() ? h->desc.weights : h->weights[b]; }
// hsddp_api.cpp: a row in the kernels' field order; the device table with its staging (allocated once);
// the table brought up to the host rows on the handle's stream (never inside a graph capture);
// the setter's check of one row (finite fields; negative weights are legal)
void weights_row(const hsddp_hkd_weights &w, Wts &r);
int ensure_weights_table(hsddp_handle h);
int sync_weights(hsddp_handle h);
bool weights_finite(const hsddp_hkd_weights &w);
// phase i of robot b: its override, or the robot's row, or the handle's
inline const hsddp_hkd_weights &weights_of(hsddp_handle h, size_t b, int i)
{
    const size_t q = b * (size_t)h->p.P + i;
    return !h->pw_set.empty() && i < h->p.P && h->pw_set[q] ? *reinterpret_cast<const hsddp_hkd_weights *>(&h->pw[q * NW])
                                                            : weights_of(h, b);
}
// hsddp_api.cpp: the per-phase device table with its staging (allocated once); the table brought up to
// the host rows on the handle's stream (never inside a graph capture); the new host rows taken
// (swapped in) after a layout change (hsddp_phases.cpp formed them); after any change of the flags:
// both emptied when no override is left, the device table due
int ensure_phase_weights_table(hsddp_handle h);
int sync_phase_weights(hsddp_handle h);
void adopt_phase_weights(hsddp_handle h, std::vector<int> &set, std::vector<double> &rows);
void settle_phase_weights(hsddp_handle h);
// every override gone (a new layout, w = NULL)
inline void drop_phase_weights(hsddp_handle h)
{
    if (h->pw_set.empty()) return;
    h->pw_set.clear();
    h->pw.clear();
    h->slots_fresh = false;
}

// phase of control slot kc in a layout
inline int phase_of_control(const Layout &L, int kc)
{
    int i = 0;
    while (i + 1 < L.P && kc >= L.k0[i + 1]) ++i;
    return i;
}

// control u of compact gain row q at control slot k of element b (KCW layout, hsddp_internal.h)
inline int coupled_control(hsddp_handle h, size_t b, size_t k, int q)
{
    const Params &p = h->p;
    const int i = phase_of_control(layout_of(h, b), (int)k);
    const int c = h->contacts[(b * (p.P + 1) + i) * 4 + q / 3];
    return c ? q : 12 + q;
}

template <typename T>
inline int dalloc(hsddp_handle h, T *&ptr, size_t n)
{
    void *p = nullptr;
    size_t sz = n * sizeof(T);
    if (sz == 0) sz = 16;
    hipError_t e = hipMalloc(&p, sz);
    if (e != hipSuccess) return fail(HSDDP_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    // zeroed on the handle's stream once it exists: the null stream is not ordered with a
    // non-blocking stream, so a null-stream memset of a buffer allocated mid-solve (the shift's
    // spares) could land after the kernel that fills it
    if (h->stream) hipMemsetAsync(p, 0, sz, h->stream);
    else {
        hipMemset(p, 0, sz);
        hipStreamSynchronize(nullptr);
    }
    h->allocs.push_back(p);
    h->bytes += sz;
    ptr = (T *)p;
    return HSDDP_OK;
}

inline int h2d(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return HSDDP_OK;
}

inline int d2h(void *dst, const void *src, size_t bytes)
{
    if (!dst) return HSDDP_OK;
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

// hsddp_api.cpp
// install per-element layouts: device records, sweep pairs (equal layouts share a wave), strides
int set_layouts(hsddp_handle h, const std::vector<Layout> &lays);
// the handle takes the shared layout L with the phases' reach flags (null: none reached): Params,
// the descriptor's n_phases / horizons; per-element layouts and their flags are dropped
void adopt_shared_layout(hsddp_handle h, const Layout &L, const int *reach);

}  // namespace hsddp
