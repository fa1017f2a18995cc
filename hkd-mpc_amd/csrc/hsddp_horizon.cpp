// hsddp_horizon.cpp — the MPC caller's side of the C-ABI, around the solve: command extraction
// (HKDMPCSolver::update_foot_placement + publish_mpc_cmd), the receding-horizon shift
// (HKDProblem::update, HKDProblem.cpp:117-222), the reference table and the per-slot references
// built from it, hsddp_advance, which steps all of them from the table,
// hsddp_restart_elements, which starts single elements again as new problems, and
// hsddp_copy_elements / _export_ / _import_, which move elements between handles.  What is here is the
// device and the handle: argument and state checks, allocations, copies, launches,
// synchronisations, buffer swaps and the handle's flags.  The bookkeeping (which phases, rows,
// slot maps, strides, pairs and clocks follow) is planned in hsddp_phases.cpp from a read-only
// view of the handle (view_of), so each entry point reads: check, plan, apply, commit.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hsddp_handle.h"
#include "hsddp_mpc.h"
#include "hsddp_restart.h"
#include "hsddp_elements.h"

using namespace hsddp;

// ---- MPC command extraction (HKDMPCSolver::update_foot_placement + publish_mpc_cmd) ----------
// ticket >= 0 (asynchronous form): the records go to device buffer `ticket` and from there to its
// pinned host buffer on the copy stream; out is unused
static int extract_commands(hsddp_handle h, int nsteps_between_mpc, double mpc_time, double dt_mpc,
                            const double *status_durations, int durations_per_element, const float *foot_placements,
                            int feet_per_element, float solve_time, hsddp_mpc_command *out, bool out_on_device,
                            int ticket = -1, bool measured = false)
{
    if (!h || (!out && ticket < 0)) return fail(HSDDP_ERR_ARG, "null argument");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (measured) {
        // the feet are the handle's device copy of the measured records', per element; NULL durations
        // are the handle's own when the references were built from a table (hsddp_get_phase_info's)
        if (!h->meas_held || !h->meas_feet)
            return fail(HSDDP_ERR_ARG, "no measured states held for this tick (hsddp_update_problem_measured)");
        foot_placements = nullptr;
        feet_per_element = 1;
        if (!status_durations && h->durations.size() == (size_t)h->p.B * h->p.P * 4) {
            status_durations = h->durations.data();
            durations_per_element = 1;
        }
    }
    const Params &p = h->p;
    CmdArgs a{};
    a.n = nsteps_between_mpc + 7;  // HKDMPC.cpp:232-233
    if (nsteps_between_mpc < 1 || a.n > HSDDP_CMD_STEPS || a.n > p.Kc)
        return fail(HSDDP_ERR_ARG, "nsteps_between_mpc + 7 must fit the command (10 rows) and the horizon");
    // the knot walk of publish_mpc_cmd (HKDMPC.cpp:239-246): s runs over phase i's controls (per-
    // element layouts: each workgroup walks its element's own)
    if (h->lays.empty())
        for (int k = 0, i = 0, s = 0; k < a.n; ++k, ++s) {
            if (s >= p.N[i]) { s = 0; ++i; }
            a.kc[k] = p.k0[i] + s;
            a.xs[k] = p.s0[i] + s;
            a.ph[k] = i;
        }
    a.mpc_time = mpc_time;
    a.dt_mpc = dt_mpc;
    a.solve_time = solve_time;
    a.dur_per_elem = durations_per_element ? 1 : 0;
    a.feet_per_elem = feet_per_element ? 1 : 0;
    HIPCHK(hipSetDevice(h->desc.device));
    const size_t B = p.B;
    const size_t cmd_bytes = (B * sizeof(hsddp_mpc_command) + 255) / 256 * 256;
    const size_t dur_bytes = status_durations ? ((a.dur_per_elem ? B : 1) * p.P * 4 * sizeof(double) + 255) / 256 * 256 : 0;
    const size_t feet_bytes = foot_placements ? (a.feet_per_elem ? B : 1) * 12 * sizeof(float) : 0;
    char *buf;
    int rc;
    if ((rc = scratch(h, cmd_bytes + dur_bytes + feet_bytes, &buf))) return rc;
    hsddp_mpc_command *dcmd = ticket >= 0 ? h->cmd_dev[ticket] : out_on_device ? out : (hsddp_mpc_command *)buf;
    const size_t dur_len = (a.dur_per_elem ? B : 1) * p.P * 4 * sizeof(double);
    const void *dur_src = status_durations, *feet_src = foot_placements;
    if (ticket >= 0 && (status_durations || foot_placements)) {
        // the call returns before the kernel runs and the caller may release its (pageable) inputs:
        // they are copied into this ticket's pinned staging first, and the H2D copies read from
        // there — nothing waits for the handle's stream.  The staging's previous copies (two
        // extractions ago) finished before that extraction's kernel, whose event is long past.
        char *&pin = h->cmd_in_host[ticket];
        if (h->cmd_in_bytes[ticket] < dur_bytes + feet_bytes) {
            HIPCHK(hipEventSynchronize(h->cmd_ready[ticket]));
            if (pin) hipHostFree(pin);
            pin = nullptr;
            h->cmd_in_bytes[ticket] = 0;
            HIPCHK(hipHostMalloc((void **)&pin, dur_bytes + feet_bytes, 0));
            h->cmd_in_bytes[ticket] = dur_bytes + feet_bytes;
        } else {
            HIPCHK(hipEventSynchronize(h->cmd_ready[ticket]));
        }
        if (status_durations) std::memcpy(pin, status_durations, dur_len);
        if (foot_placements) std::memcpy(pin + dur_bytes, foot_placements, feet_bytes);
        dur_src = pin;
        feet_src = pin + dur_bytes;
    }
    if (status_durations) {
        a.durations = (const double *)(buf + cmd_bytes);
        if ((rc = h2d((void *)a.durations, dur_src, dur_len, h->stream))) return rc;
    }
    if (foot_placements) {
        a.feet = (const float *)(buf + cmd_bytes + dur_bytes);
        if ((rc = h2d((void *)a.feet, feet_src, feet_bytes, h->stream))) return rc;
    }
    if (measured) a.feet = h->meas_feet;
    if (ticket >= 0)  // the buffer's previous copy (two extractions ago) has left it
        HIPCHK(hipStreamWaitEvent(h->stream, h->cmd_copied[ticket], 0));
    launch_extract_commands(p, h->d, a, dcmd, h->stream);
    HIPCHK(hipGetLastError());
    if (ticket >= 0) {  // D2H on the copy stream, behind the kernel: the handle's stream moves on
        HIPCHK(hipEventRecord(h->cmd_ready[ticket], h->stream));
        HIPCHK(hipStreamWaitEvent(h->copy_stream, h->cmd_ready[ticket], 0));
        HIPCHK(hipMemcpyAsync(h->cmd_host[ticket], dcmd, B * sizeof(hsddp_mpc_command), hipMemcpyDeviceToHost,
                              h->copy_stream));
        HIPCHK(hipEventRecord(h->cmd_copied[ticket], h->copy_stream));
        return HSDDP_OK;
    }
    if (!out_on_device) HIPCHK(hipMemcpyAsync(out, dcmd, B * sizeof(hsddp_mpc_command), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return HSDDP_OK;
}

extern "C" int hsddp_extract_commands(hsddp_handle h, int nsteps_between_mpc, double mpc_time, double dt_mpc,
                                      const double *status_durations, int durations_per_element,
                                      const float *foot_placements, int feet_per_element, float solve_time,
                                      hsddp_mpc_command *out)
{
    return extract_commands(h, nsteps_between_mpc, mpc_time, dt_mpc, status_durations, durations_per_element,
                            foot_placements, feet_per_element, solve_time, out, false);
}

extern "C" int hsddp_extract_commands_device(hsddp_handle h, int nsteps_between_mpc, double mpc_time, double dt_mpc,
                                             const double *status_durations, int durations_per_element,
                                             const float *foot_placements, int feet_per_element, float solve_time,
                                             void *out_device)
{
    return extract_commands(h, nsteps_between_mpc, mpc_time, dt_mpc, status_durations, durations_per_element,
                            foot_placements, feet_per_element, solve_time, (hsddp_mpc_command *)out_device, true);
}

extern "C" int hsddp_extract_commands_measured(hsddp_handle h, int nsteps_between_mpc, double mpc_time, double dt_mpc,
                                               const double *status_durations, int durations_per_element,
                                               float solve_time, hsddp_mpc_command *out, int out_on_device)
{
    return extract_commands(h, nsteps_between_mpc, mpc_time, dt_mpc, status_durations, durations_per_element, nullptr,
                            1, solve_time, out, out_on_device != 0, -1, true);
}

extern "C" int hsddp_extract_commands_async(hsddp_handle h, int nsteps_between_mpc, double mpc_time, double dt_mpc,
                                            const double *status_durations, int durations_per_element,
                                            const float *foot_placements, int feet_per_element, float solve_time,
                                            int *ticket)
{
    if (!h || !ticket) return fail(HSDDP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->desc.device));
    const size_t bytes = (size_t)h->p.B * sizeof(hsddp_mpc_command);
    if (!h->copy_stream) {  // first use: two record buffers on each side, the copy stream, events
        HIPCHK(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
        for (int q = 0; q < 2; ++q) {
            HIPCHK(hipMalloc((void **)&h->cmd_dev[q], bytes));
            HIPCHK(hipHostMalloc((void **)&h->cmd_host[q], bytes, 0));
            HIPCHK(hipEventCreateWithFlags(&h->cmd_ready[q], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->cmd_copied[q], hipEventDisableTiming));
            HIPCHK(hipEventRecord(h->cmd_copied[q], h->copy_stream));
        }
    }
    const int t = h->cmd_next;
    const int rc = extract_commands(h, nsteps_between_mpc, mpc_time, dt_mpc, status_durations, durations_per_element,
                                    foot_placements, feet_per_element, solve_time, nullptr, false, t);
    if (rc) return rc;
    h->cmd_next ^= 1;
    *ticket = t;
    return HSDDP_OK;
}

extern "C" int hsddp_commands_wait(hsddp_handle h, int ticket, const hsddp_mpc_command **records)
{
    if (!h || !records) return fail(HSDDP_ERR_ARG, "null argument");
    if (ticket < 0 || ticket > 1 || !h->copy_stream) return fail(HSDDP_ERR_ARG, "no such extraction ticket");
    HIPCHK(hipEventSynchronize(h->cmd_copied[ticket]));
    *records = h->cmd_host[ticket];
    return HSDDP_OK;
}

// ---- receding-horizon shift (HKDProblem::update, HKDProblem.cpp:117-222) ----------------------
// The shift on the device and in the handle.  When every element ends on one layout the handle
// keeps (or returns to) the shared layout.  A phase that would carry more than HSDDP_MAX_TD
// touchdown constraints keeps the first ones (the shift is otherwise complete):
// HSDDP_ERR_UNSUPPORTED, or, with `overflow`, *overflow = 1 and HSDDP_OK (hsddp_advance finishes
// the step and reports it then).  defer: no synchronisation (one layout for the batch; the flag is
// read by hsddp_advance).  zero_u0 = false: a plan of no steps that only moves rows to new strides
// (hsddp_restart_elements) leaves Ubar[0] as it is.
static int shift_apply(hsddp_handle h, const ShiftPlan &plan, bool defer, int *overflow, bool zero_u0 = true)
{
    h->slots_fresh = false;
    Params &p = h->p;
    const size_t B = p.B;
    const std::vector<int> &map_id = plan.map_id;
    const int nk = (int)plan.phs.size();
    ShiftMaps m;
    std::string why;
    int rc;
    if ((rc = flatten_shift(plan, p.Kc, h->S_cap, m, why))) return fail(rc, why);
    const int Snew = m.S_new, Pnew = m.P_new;
    // the terrain rows follow the phases on the host (the old rows are read before the layouts change)
    std::vector<double> terrain;
    if (!h->terrain.empty()) shift_terrain(view_of(h), plan, Pnew, terrain);
    // ... and the weight overrides (a phase the steps started has none)
    const bool had_pw = !h->pw_set.empty();
    std::vector<int> pw_set;
    std::vector<double> pw_rows;
    if (had_pw) shift_phase_weights(view_of(h), plan, Pnew, pw_set, pw_rows);
    std::vector<int> &smap = m.smap, &cmap = m.cmap, &rmap = m.rmap, &pmap = m.pmap, &nadd = m.nadd;
    HIPCHK(hipSetDevice(h->desc.device));
    Bufs &d = h->d;
    if (!h->spare_K) {  // (the new Xbar / Ubar rows go to each element's third buffer)
        void *sk;
        if (p.fp32) { float *k32; if ((rc = dalloc(h, k32, B * p.Kc * KCW))) return rc; sk = k32; }
        else { double *k64; if ((rc = dalloc(h, k64, B * p.Kc * KCW))) return rc; sk = k64; }
        h->spare_K = sk;
    }
    if (!h->spare_reb_delta) {
        if ((rc = dalloc(h, h->spare_reb_delta, B * p.Kc * 20)) || (rc = dalloc(h, h->spare_reb_eps, B * p.Kc * 20)) ||
            (rc = dalloc(h, h->spare_al_sigma, B * HSDDP_MAX_PHASES * MTD * 4)) ||
            (rc = dalloc(h, h->spare_al_lambda, B * HSDDP_MAX_PHASES * MTD * 4)) ||
            (rc = dalloc(h, h->spare_td_mask, B * HSDDP_MAX_PHASES * MTD)) ||
            (rc = dalloc(h, h->spare_cf_u, B * p.Kc * 12)) || (rc = dalloc(h, h->spare_cf_flag, B * p.Kc)))
            return rc;
    }
    if (!h->spare_dX) {
        if ((rc = dalloc(h, h->spare_dX, B * h->S_cap * NX)) || (rc = dalloc(h, h->spare_dU, B * p.Kc * NX)) ||
            (rc = dalloc(h, h->spare_du, B * p.Kc * NX)))
            return rc;
    }
    char *buf;
    const size_t nmaps = smap.size() + cmap.size() + rmap.size() + pmap.size() + nadd.size();
    if ((rc = scratch(h, (nmaps + (nk > 1 ? B : 0)) * sizeof(int), &buf))) return rc;
    int *dsm = (int *)buf, *dcm = dsm + smap.size(), *drm = dcm + cmap.size(), *dpm = drm + rmap.size(),
        *dna = dpm + pmap.size(), *did = dna + nadd.size();
    if ((rc = h2d(dsm, smap.data(), smap.size() * sizeof(int), h->stream)) ||
        (rc = h2d(dcm, cmap.data(), cmap.size() * sizeof(int), h->stream)) ||
        (rc = h2d(drm, rmap.data(), rmap.size() * sizeof(int), h->stream)) ||
        (rc = h2d(dpm, pmap.data(), pmap.size() * sizeof(int), h->stream)) ||
        (rc = h2d(dna, nadd.data(), nadd.size() * sizeof(int), h->stream)) ||
        (nk > 1 && (rc = h2d(did, map_id.data(), B * sizeof(int), h->stream))))
        return rc;
    // the constraint parameters first (they read the old layout's strides)
    ShiftParamArgs pa;
    pa.Kc = p.Kc; pa.P_old = p.P; pa.P_new = Pnew;
    pa.rmap = drm; pa.cmap = dcm; pa.pmap = dpm; pa.nadd = dna;
    pa.map_id = nk > 1 ? did : nullptr;
    pa.reb_delta0 = p.grf_delta; pa.reb_eps0 = p.grf_eps; pa.td_sigma0 = p.td_sigma; pa.td_lambda0 = p.td_lambda;
    pa.overflow = d.counter + 6;
    HIPCHK(hipMemsetAsync(d.counter + 6, 0, sizeof(int), h->stream));
    ShiftParamOut po;
    po.reb_delta = h->spare_reb_delta; po.reb_eps = h->spare_reb_eps; po.al_sigma = h->spare_al_sigma;
    po.al_lambda = h->spare_al_lambda; po.td_mask = h->spare_td_mask; po.cf_u = h->spare_cf_u;
    po.cf_flag = h->spare_cf_flag;
    launch_shift_params(p.B, pa, d, po, h->stream);
    HIPCHK(hipMemcpyAsync(h->host_counter + 6, d.counter + 6, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    ShiftArgs a;
    a.S_old = p.S; a.S_new = Snew; a.Kc = p.Kc;
    a.smap = dsm; a.cmap = dcm;
    a.map_id = nk > 1 ? did : nullptr;
    a.fp32 = p.fp32;
    a.zero_u0 = zero_u0 ? 1 : 0;  // trajectory_ptrs.front()->Ubar[0].setZero() (HKDProblem.cpp:219)
    a.stage = nullptr;
    if (Snew != p.S) {
        if (!h->shift_stage && (rc = dalloc(h, h->shift_stage, 3 * B * h->S_cap * NX))) return rc;
        a.stage = h->shift_stage;
    }
    a.dX_new = h->spare_dX; a.dU_new = h->spare_dU; a.du_new = h->spare_du;
    launch_shift_gather(p.B, a, d, h->spare_K, h->stream);  // (working rows, search direction and sel too)
    HIPCHK(hipGetLastError());
    // defer (hsddp_advance, one layout for the batch): the caller's host work runs under the gather;
    // everything after it is ordered on the handle's stream
    const bool async = defer && nk == 1;
    if (!async) HIPCHK(hipStreamSynchronize(h->stream));
    std::swap(d.reb_delta, h->spare_reb_delta);
    std::swap(d.reb_eps, h->spare_reb_eps);
    std::swap(d.al_sigma, h->spare_al_sigma);
    std::swap(d.al_lambda, h->spare_al_lambda);
    std::swap(d.td_mask, h->spare_td_mask);
    std::swap(d.cf_u, h->spare_cf_u);
    std::swap(d.cf_flag, h->spare_cf_flag);
    std::swap(d.dX, h->spare_dX);
    std::swap(d.dU, h->spare_dU);
    std::swap(d.du, h->spare_du);
    const bool td_overflow = !async && h->host_counter[6] != 0;
    if (p.fp32) { float *t = d.K32; d.K32 = (float *)h->spare_K; h->spare_K = t; }
    else { double *t = d.K; d.K = (double *)h->spare_K; h->spare_K = t; }
    // the new layouts
    if (nk == 1) {  // one layout for the batch: the handle's own
        int reach[HSDDP_MAX_PHASES];
        plan.reach(0, reach);
        adopt_shared_layout(h, plan.nl[0], reach);
    } else {
        std::vector<Layout> lays;
        std::vector<int> reach;
        shifted_layouts(plan, lays, reach);
        if ((rc = set_layouts(h, lays))) return rc;
        h->reach_el.swap(reach);
    }
    if (!h->terrain.empty()) {
        h->terrain.swap(terrain);
        h->terrain_stale = true;
    }
    if (had_pw) adopt_phase_weights(h, pw_set, pw_rows);
    h->need_inputs = true;
    h->refs_on_device = false;  // built for the old layout
    h->ref_cols_stale = true;
    h->contacts_current = false;
    if (async) {
        h->shift_overflow_pending = true;
        h->scratch_reserved = ((nmaps + (nk > 1 ? B : 0)) * sizeof(int) + 255) & ~(size_t)255;
        for (std::vector<int> *v : {&smap, &cmap, &rmap, &pmap, &nadd}) h->shift_keep.push_back(std::move(*v));
    }
    if (td_overflow) {  // the shift itself is complete; the constraints past HSDDP_MAX_TD were not added
        if (overflow) *overflow = 1;
        else return fail(HSDDP_ERR_UNSUPPORTED, "a phase would carry more than HSDDP_MAX_TD touchdown constraints");
    }
    return HSDDP_OK;
}

// the shift of every element by the caller's flags: cc[b * bstride + j] is element b's flag of step j
static int shift_by_flags(hsddp_handle h, int n_steps, const int *cc, size_t bstride)
{
    if (!h || (n_steps > 0 && !cc)) return fail(HSDDP_ERR_ARG, "null argument");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (n_steps < 0) return fail(HSDDP_ERR_ARG, "n_steps must be >= 0");
    h->slots_fresh = false;
    ShiftPlan plan;
    std::string why;
    // (every refusal comes before any device work: the handle stays usable)
    if (int rc = plan_shift(view_of(h), n_steps, cc, bstride, plan, why)) return fail(rc, why);
    h->sim_shifted += n_steps;  // (hsddp_update_problem_simulated compares it with the simulation's steps)
    return shift_apply(h, plan, false, nullptr);
}

extern "C" int hsddp_shift(hsddp_handle h, int n_steps, const int *contact_change)
{
    return shift_by_flags(h, n_steps, contact_change, 0);
}

extern "C" int hsddp_shift_elements(hsddp_handle h, int n_steps, const int *contact_change)
{
    return shift_by_flags(h, n_steps, contact_change, h ? (size_t)n_steps : 0);
}

// (the hash in the element records' compatibility key, hsddp_elements.h)
static unsigned long long fnv1a(const void *data, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)data)[i]) * 1099511628211ull;
    return h;
}

// ---- batched reference construction ------------------------------------------------------------
extern "C" int hsddp_set_reference_table(hsddp_handle h, const hsddp_quad_state *table, int n, float dt_ref)
{
    if (!h || !table || n < 1) return fail(HSDDP_ERR_ARG, "null / empty table");
    if (!(dt_ref > 0)) return fail(HSDDP_ERR_ARG, "dt_ref must be > 0");
    HIPCHK(hipSetDevice(h->desc.device));
    std::vector<double> t((size_t)n * RT_W, 0.0);
    for (int i = 0; i < n; ++i) {
        double *q = &t[(size_t)i * RT_W];
        const hsddp_quad_state &s = table[i];
        for (int j = 0; j < 12; ++j) {
            q[RT_BODY + j] = s.body_state[j]; q[RT_QJ + j] = s.qJ[j]; q[RT_QJD + j] = s.qJd[j];
            q[RT_FOOT + j] = s.foot_placements[j]; q[RT_GRF + j] = s.grf[j];
        }
        for (int l = 0; l < 4; ++l) q[RT_C + l] = s.contact[l];
    }
    if (h->ref_table) { hipFree(h->ref_table); h->ref_table = nullptr; }
    HIPCHK(hipMalloc((void **)&h->ref_table, t.size() * sizeof(double)));
    HIPCHK(hipMemcpy(h->ref_table, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    h->ref_n = n;
    h->ref_dt = dt_ref;
    h->table_host.assign(table, table + n);
    h->table_key = fnv1a(table, (size_t)n * sizeof(hsddp_quad_state));
    h->win_start.clear();
    return HSDDP_OK;
}

// initial: a new problem (not an hsddp_advance step): QuadReference's clock restarts and every
// phase's contact duration is read at its start time, as HKDProblem::initialization does
// (get_contact_duration_at_t at t = 0 and at each phase end, HKDProblem.cpp:38,63)
static int build_refs(hsddp_handle h, const int *window_start, int window_len, const float *phase_start_times,
                      float dt_sim, bool initial)
{
    if (!h || !window_start) return fail(HSDDP_ERR_ARG, "null argument");
    if (!h->ref_table) return fail(HSDDP_ERR_ARG, "no reference table (hsddp_set_reference_table)");
    if (window_len < 1 || !(dt_sim > 0)) return fail(HSDDP_ERR_ARG, "window_len >= 1 and dt_sim > 0 required");
    const Params &p = h->p;
    const int Br = h->Bref;
    const bool elem = !h->lays.empty();
    for (int b = 0; b < Br; ++b)
        if (window_start[b] < 0 || window_start[b] >= h->ref_n) return fail(HSDDP_ERR_ARG, "window start outside the table");
    if (elem && phase_start_times)
        return fail(HSDDP_ERR_ARG, "per-element layouts: the phase start times follow each element's own float clock (NULL)");
    // one slot map per distinct layout ([n_maps][S], padding slots repeat the last sample), the phases
    // starting at the caller's times or on the float clock
    RefPlan rp;
    plan_refs(view_of(h), window_start, window_len, phase_start_times, dt_sim, initial, rp);
    const std::vector<int> &idx = rp.idx, &map_id = rp.map_id;
    HIPCHK(hipSetDevice(h->desc.device));
    char *buf;
    int rc;
    if ((rc = scratch(h, h->scratch_reserved + (Br + idx.size() + map_id.size()) * sizeof(int), &buf))) return rc;
    buf += h->scratch_reserved;  // (after a pending shift's maps: hsddp_advance)
    int *dstart = (int *)buf, *didx = dstart + Br, *dmap = didx + idx.size();
    if ((rc = h2d(dstart, window_start, Br * sizeof(int), h->stream)) ||
        (rc = h2d(didx, idx.data(), idx.size() * sizeof(int), h->stream)) ||
        (elem && (rc = h2d(dmap, map_id.data(), map_id.size() * sizeof(int), h->stream))))
        return rc;
    RefArgs a{h->ref_table, h->ref_n, dstart, didx, elem ? dmap : nullptr};
    launch_build_refs(p, h->d, Br, a, h->stream);
    h->ref_cols_stale = false;  // (k_build_refs writes the entry-major copy too)
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->refs_on_device = true;
    h->win_start.assign(window_start, window_start + Br);
    h->win_len = window_len;
    h->dt_sim = dt_sim;
    if (initial) {
        h->t_cur = 0;
        h->t_el.clear();
        h->durations.swap(rp.durations);
    }
    return HSDDP_OK;
}

extern "C" int hsddp_build_references(hsddp_handle h, const int *window_start, int window_len,
                                      const float *phase_start_times, float dt_sim)
{
    if (h) h->slots_fresh = false;  // new reference rows: the running costs change
    return build_refs(h, window_start, window_len, phase_start_times, dt_sim, true);
}

// ---- reference-driven receding-horizon step -------------------------------------------------------
// HKDProblem::update (HKDProblem.cpp:117-222) with the contacts read from the reference table:
// per simulation step the window advances (QuadReference::step, QuadReference.cpp:33-47), the
// contact at the new horizon end (get_contact_at_t(new_end - new_start)) decides whether the last
// phase grows or a new phase starts, and a last phase that has reached its end gets the touchdown
// constraint / reset map towards the contact at plan_duration + dt_mpc (add_tconstr_one_phase,
// :199-202, 268-308).  Then the shifted warm start (hsddp_shift), the new layout's references
// (build_refs) and the new contacts and x0 (hsddp_update_problem).
static int advance_impl(hsddp_handle h, int n_steps, float plan_duration, float dt_mpc, const double *x0,
                        int *contact_change, int &overflow)
{
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (h->need_inputs) return fail(HSDDP_ERR_ARG, "the previous shift awaits hsddp_update_problem");
    if (h->win_start.empty() || h->table_host.empty())
        return fail(HSDDP_ERR_ARG, "references not built from a table (hsddp_build_references)");
    if (n_steps < 0) return fail(HSDDP_ERR_ARG, "n_steps must be >= 0");
    // HSDDP_ADVANCE_TIMING=1: wall time of the advance's stages to stderr (a diagnostic)
    static const bool timing = std::getenv("HSDDP_ADVANCE_TIMING") != nullptr;
    using clk = std::chrono::steady_clock;
    clk::time_point tmark = clk::now();
    double tstage[5] = {0, 0, 0, 0, 0};
    auto stage = [&](int q) {
        if (!timing) return;
        const clk::time_point t = clk::now();
        tstage[q] = std::chrono::duration<double, std::micro>(t - tmark).count();
        tmark = t;
    };
    // plan: the walk over the table (every refusal of the step comes here, before the handle changes)
    const HorizonView v = view_of(h);
    AdvanceWalk w;
    std::string why;
    int rc;
    if ((rc = walk_advance(v, n_steps, plan_duration, w, why))) return fail(rc, why);
    stage(0);
    // apply: the shift, deferred when the batch agrees on one slot map (a touchdown overflow is
    // reported after the rest of the step either way); the new rows are formed under its gather, at
    // the new stride (v still points at the old rows, which the shift leaves alone)
    h->sim_shifted += n_steps;  // (hsddp_update_problem_simulated compares it with the simulation's steps)
    if ((rc = shift_apply(h, w.plan, w.agree, &overflow))) return rc;
    stage(1);
    std::vector<int> contacts;
    std::vector<double> dur;
    advance_rows(v, w, h->p.P, plan_duration, dt_mpc, contacts, dur);
    stage(2);
    if ((rc = build_refs(h, w.ws.data(), h->win_len, nullptr, h->dt_sim, false))) return rc;
    stage(3);
    // commit: contacts (with x0, or held for the update that brings it), durations, clocks
    if (x0) {
        if ((rc = hsddp_update_problem(h, contacts.data(), x0, nullptr, nullptr, nullptr))) return rc;
    } else {  // x0 follows from the new first phase's contact: hsddp_update_problem(h, NULL, x0, NULL...)
        h->contacts.swap(contacts);
        h->contacts_current = true;
    }
    h->durations.swap(dur);
    if (h->t_el.empty()) h->t_cur = w.t_cur[0];
    else h->t_el = w.t_cur;
    stage(4);
    if (timing)
        std::fprintf(stderr, "hsddp_advance us: bookkeeping %.1f shift %.1f contacts %.1f refs %.1f update %.1f\n",
                     tstage[0], tstage[1], tstage[2], tstage[3], tstage[4]);
    if (contact_change)  // per step: some element saw a contact change (the batch's flag when it agrees)
        std::copy(w.flags.begin(), w.flags.end(), contact_change);
    return HSDDP_OK;
}

// hsddp_advance = advance_impl, then: the deferred shift's stream is drained before the host rows its
// copies read are released (whatever path left advance_impl), and its touchdown-overflow flag is
// read.  A touchdown overflow on a complete step (both shift paths) returns HSDDP_ERR_UNSUPPORTED
// with the handle ready to solve: new layout, references, contacts, x0, durations and clock, the
// phase keeping its first HSDDP_MAX_TD touchdown constraints.  When the step failed for another
// reason, that error is returned and an overflow is added to its message.
extern "C" int hsddp_advance(hsddp_handle h, int n_steps, float plan_duration, float dt_mpc, const double *x0,
                             int *contact_change)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    int overflow = 0;
    const int rc = advance_impl(h, n_steps, plan_duration, dt_mpc, x0, contact_change, overflow);
    if (h->shift_overflow_pending) {  // the deferred shift's flag (its copy is queued on the stream)
        const hipError_t e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess && h->host_counter[6] != 0) overflow = 1;
        h->shift_overflow_pending = false;
        h->shift_keep.clear();
        h->scratch_reserved = 0;
        if (e != hipSuccess && rc == HSDDP_OK) return fail(HSDDP_ERR_DEVICE, std::string("advance: ") + hipGetErrorString(e));
    }
    static const char *msg = "a phase would carry more than HSDDP_MAX_TD touchdown constraints";
    if (rc == HSDDP_OK) return overflow ? fail(HSDDP_ERR_UNSUPPORTED, msg) : HSDDP_OK;
    if (overflow) fail(rc, std::string(hsddp_last_error()) + " (and " + msg + ")");
    return rc;
}

// ---- single elements started again (HKDProblem::initialization for a subset) -------------------
// The sweep pairs (Bufs::pairs: two elements of one layout per wave) after the listed elements of a
// per-element handle took new layouts (hsddp_handle_t::lays), patched in place: a listed element
// leaves its pair (its partner stays alone), the listed elements pair up among themselves by new
// layout, emptied entries are filled from the end.  Only the entries that change go to the device.
// (The next set_layouts — every shift of a per-element handle — pairs the whole batch afresh.)
static int repair_pairs(hsddp_handle h, const std::vector<int> &list)
{
    int np = h->p.n_pairs, rc;
    const std::vector<int> touched = patch_pairs(h->pairs_host, h->pair_of, np, h->lays.data(), list);
    if ((size_t)np > (size_t)h->p.B) return fail(HSDDP_ERR_ARG, "sweep pairs exceed the batch");
    for (int q : touched)
        if (q < np && (rc = h2d((int *)h->d.pairs + 2 * q, &h->pairs_host[2 * q], 2 * sizeof(int), h->stream))) return rc;
    h->p.n_pairs = np;
    return HSDDP_OK;
}

// The host side of hsddp_restart_elements: every listed element's window segmented anew
// (plan_restart, hsddp_phases.cpp), its layout, contact rows, durations, window start and clock
// replaced, and the device rows of a new problem written for the listed elements only
// (hsddp_restart.hip).  The per-phase and per-slot buffers are strided by the batch's largest P and
// S: when the restart changes either, the other elements' rows move to the new strides first, by
// the shift's gather with identity slot maps (no step), and the references are rebuilt at the new
// stride — one pass over the batch, as a shift is; otherwise nothing of another element is touched.
// Every refusal comes before the first change to the handle.
extern "C" int hsddp_restart_elements(hsddp_handle h, const int *mask, const int *window_start, float plan_duration,
                                      float dt_mpc, const double *x0)
{
    if (!h || !mask || !window_start) return fail(HSDDP_ERR_ARG, "null argument");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (!h->ref_table || h->win_start.empty() || h->table_host.empty())
        return fail(HSDDP_ERR_UNSUPPORTED, "references not built from a table (hsddp_set_reference_table + "
                                           "hsddp_build_references)");
    Params &p = h->p;
    const int B = p.B, Br = h->Bref;
    const std::vector<int> list = listed_elements(mask, B);
    const int n = (int)list.size();
    if (n == 0) return HSDDP_OK;  // nothing restarts: nothing is launched, nothing changes
    if (n != B && Br == 1)
        return fail(HSDDP_ERR_UNSUPPORTED, "shared references: a restart of some elements needs per-element references "
                                           "(ref_per_element = 1)");
    if (!h->refs_on_device || !h->contacts_current || h->contacts.size() != (size_t)B * (p.P + 1) * 4 ||
        h->durations.size() != (size_t)B * p.P * 4)
        return fail(HSDDP_ERR_ARG, "no references and contacts of the current layout on the handle (after hsddp_shift: "
                                   "hsddp_build_references and hsddp_update_problem first)");
    // plan: the listed elements' new problems and what they mean for the batch (strides, layouts,
    // rows, slot maps, clocks); every refusal comes here
    RestartBatch r;
    std::string why;
    int rc;
    if ((rc = plan_restart_batch(view_of(h), list, window_start, plan_duration, dt_mpc, r, why))) return fail(rc, why);
    const bool restride = r.restride, in_place = r.in_place;
    // apply
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (restride) {  // the other elements' rows to the new strides (installs per-element layouts)
        const bool pending = h->need_inputs;
        if ((rc = shift_apply(h, r.stride_plan, false, nullptr, false))) return rc;
        h->need_inputs = pending;
    }
    if (r.one) {
        const int none[HSDDP_MAX_PHASES] = {0};
        adopt_shared_layout(h, r.plans[0].L, none);
    } else if (in_place) {
        for (int m = 0; m < n; ++m) {  // (the device records go with the restart's kernel)
            h->lays[list[m]] = r.plans[m].L;
            std::fill_n(&h->reach_el[(size_t)list[m] * HSDDP_MAX_PHASES], HSDDP_MAX_PHASES, 0);
        }
        if ((rc = repair_pairs(h, list))) return rc;
    } else if (!restride) {
        if ((rc = set_layouts(h, r.lays))) return rc;
        h->reach_el.swap(r.reach);
    }
    // contact rows [B][P + 1][4] and durations [B][P][4]: the listed elements' new; at a new stride
    // the others' rows have moved
    if (restride) {
        h->contacts.swap(r.contacts);
        h->durations.swap(r.durations);
    } else {
        for (int m = 0; m < n; ++m)
            put_restart_rows(r.plans[m], p.P, &h->contacts[(size_t)list[m] * (p.P + 1) * 4],
                             &h->durations[(size_t)list[m] * p.P * 4]);
    }
    h->contacts_current = true;
    if (!h->terrain.empty()) {  // a new problem's terrain is the handle's cparams, as on a new handle
        const HorizonView v = view_of(h);
        for (int m = 0; m < n; ++m) put_terrain_rows(nullptr, 0, p.P, v.fill, &h->terrain[(size_t)list[m] * p.P * 2]);
        h->terrain_stale = true;
    }
    if (!h->pw_set.empty()) {  // a new problem's cost objects are new: no overrides (the robot's row stays)
        for (int m = 0; m < n; ++m)  // (in place: only the restarted robots' rows are written)
            put_phase_weight_rows(nullptr, nullptr, 0, p.P, &h->pw_set[(size_t)list[m] * p.P], &h->pw[(size_t)list[m] * p.P * NW]);
        settle_phase_weights(h);
    }
    if (restride && (rc = h2d((void *)h->d.contacts, h->contacts.data(), h->contacts.size() * sizeof(int), h->stream)))
        return rc;
    // the window starts; references: at a new stride every element's are rebuilt; shared ones (every
    // element restarts) are built as a whole; else the kernel forms the listed elements' own
    h->win_start = r.win_start;
    if (restride || Br == 1) {
        if ((rc = build_refs(h, r.win_start.data(), h->win_len, nullptr, h->dt_sim, false))) return rc;
    }
    // the clocks: QuadReference's t_cur restarts for the listed elements
    if (r.all) h->t_cur = 0;
    h->t_el.swap(r.t_el);
    // the device rows: list, window starts, slot maps (one per distinct new layout), contact rows, x0
    const std::vector<int> &idx = r.slots.idx, &map_id = r.map_id, &start = r.start, &rows = r.rows;
    std::vector<Layout> recs;  // the listed elements' layout records (in place: written by the kernel)
    if (in_place)
        for (int m = 0; m < n; ++m) recs.push_back(r.plans[m].L);
    const size_t nl = recs.size() * (sizeof(Layout) / sizeof(int));
    const size_t ni = (size_t)3 * n + idx.size() + rows.size() + nl, ib = (ni * sizeof(int) + 255) & ~(size_t)255;
    char *buf;
    if ((rc = scratch(h, ib + (x0 ? (size_t)n * NX * sizeof(double) : 0), &buf))) return rc;
    int *dl = (int *)buf, *ds = dl + n, *dm = ds + n, *di = dm + n, *dc = di + idx.size(), *dr = dc + rows.size();
    double *dx = (double *)(buf + ib);
    std::vector<double> xs;
    if (x0) {
        xs.resize((size_t)n * NX);
        for (int m = 0; m < n; ++m) std::copy_n(x0 + (size_t)list[m] * NX, NX, &xs[(size_t)m * NX]);
    }
    if ((rc = h2d(dl, list.data(), n * sizeof(int), h->stream)) || (rc = h2d(ds, start.data(), n * sizeof(int), h->stream)) ||
        (rc = h2d(dm, map_id.data(), n * sizeof(int), h->stream)) ||
        (rc = h2d(di, idx.data(), idx.size() * sizeof(int), h->stream)) ||
        (rc = h2d(dc, rows.data(), rows.size() * sizeof(int), h->stream)) ||
        (nl && (rc = h2d(dr, recs.data(), nl * sizeof(int), h->stream))) ||
        (x0 && (rc = h2d(dx, xs.data(), xs.size() * sizeof(double), h->stream))))
        return rc;
    RestartArgs a{};
    a.n = n; a.list = dl; a.start = ds; a.map_id = dm; a.slot_idx = di; a.contacts = dc;
    a.x0 = x0 ? dx : nullptr;
    a.table = h->ref_table; a.table_n = h->ref_n;
    a.build_refs = Br == 1 ? 0 : 1;
    a.lay = nl ? (const Layout *)dr : nullptr;
    // HSDDP_RESTART_TIMING=1: the kernels' device time (HIP events) to stderr (a diagnostic)
    static const bool timing = std::getenv("HSDDP_RESTART_TIMING") != nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timing) {
        HIPCHK(hipEventCreate(&ev[0]));
        HIPCHK(hipEventCreate(&ev[1]));
        HIPCHK(hipEventRecord(ev[0], h->stream));
    }
    launch_restart(p, h->d, a, h->stream);
    HIPCHK(hipGetLastError());
    if (timing) HIPCHK(hipEventRecord(ev[1], h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // (the pageable host rows above are read until here)
    if (timing) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        hipEventDestroy(ev[0]);
        hipEventDestroy(ev[1]);
        std::fprintf(stderr, "hsddp_restart_elements kernels ms: %.4f (B %d, restarted %d%s)\n", ms, B, n,
                     in_place ? ", in place" : restride ? ", new strides" : "");
    }
    // what the handle caches of rows and layouts: the slot costs are recomputed by the next k_lq, a
    // simulation held and this tick's measured foot placements are of the old problems; the
    // iteration graphs are keyed on Params / Bufs and re-captured when the layouts changed them
    h->slots_fresh = false;
    h->sim_fresh = false;
    h->meas_held = false;
    if (!x0) h->need_inputs = true;  // as hsddp_advance with x0 = NULL leaves them
    return HSDDP_OK;
}

// ---- elements moved between slots, handles and host records ----------------------------------------
// hsddp_copy_elements, hsddp_export_elements, hsddp_import_elements: an element's whole between-tick
// state copied from a slot of one live handle to a slot of another (or the same), directly or
// through a host record.  The receiving side is hsddp_restart_elements' machinery (layouts patched
// in place, repair_pairs, the restride pass, per-element clocks, a compacted list driving the
// kernels) with the rows read from the source (hsddp_elements.hip) instead of built anew.
static bool table_driven(hsddp_handle h) { return h->ref_table && !h->win_start.empty() && !h->table_host.empty(); }

static ElementKey key_of(hsddp_handle h)
{
    ElementKey k;
    std::memset(&k, 0, sizeof k);
    k.Kc = h->p.Kc; k.fp32 = h->p.fp32; k.S_cap = (int)h->S_cap; k.dt = h->desc.dt;
    k.weights = fnv1a(&h->desc.weights, sizeof h->desc.weights);
    k.cparams = fnv1a(&h->desc.cparams, sizeof h->desc.cparams);
    k.has_table = table_driven(h) ? 1 : 0;
    if (k.has_table) {
        k.table = h->table_key; k.ref_n = h->ref_n; k.ref_dt = h->ref_dt; k.win_len = h->win_len; k.dt_sim = h->dt_sim;
    }
    return k;
}

// may an element of a handle (or record) with key s continue in a handle with key d?
static int compatible(const ElementKey &s, const ElementKey &d, bool records)
{
    if (s.Kc != d.Kc) return fail(HSDDP_ERR_ARG, "the element's Kc is not the destination's");
    if (s.dt != d.dt) return fail(HSDDP_ERR_ARG, "the element's dt is not the destination's");
    if (s.fp32 != d.fp32) return fail(HSDDP_ERR_ARG, "the element's precision mode (riccati_fp32) is not the destination's");
    if (s.weights != d.weights || s.cparams != d.cparams)
        return fail(HSDDP_ERR_ARG, "the element's weights or constraint parameters are not the destination's");
    if (records && s.S_cap != d.S_cap) return fail(HSDDP_ERR_ARG, "the record's size is not the destination's");
    if (s.has_table != d.has_table)
        return fail(HSDDP_ERR_UNSUPPORTED, "only one of the two sides drives its references from a table");
    if (s.has_table && (s.table != d.table || s.ref_n != d.ref_n || s.ref_dt != d.ref_dt || s.win_len != d.win_len ||
                        s.dt_sim != d.dt_sim))
        return fail(HSDDP_ERR_UNSUPPORTED, "the two sides' reference tables, window lengths or simulation steps differ");
    return HSDDP_OK;
}

// a handle that can give or take an element: a problem uploaded, no inputs pending, the contact rows
// of the current layout on the host
static int settled(hsddp_handle h, const char *side)
{
    const Params &p = h->p;
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, std::string(side) + ": upload the problem first");
    if (h->need_inputs) return fail(HSDDP_ERR_ARG, std::string(side) + ": a shift, advance or restart awaits its inputs");
    if (!h->contacts_current || h->contacts.size() != (size_t)p.B * (p.P + 1) * 4)
        return fail(HSDDP_ERR_ARG, std::string(side) + ": no contacts of the current layout on the handle");
    return HSDDP_OK;
}

// the handle's host state with the durations only where they are the current layout's
static HorizonView element_view(hsddp_handle h)
{
    HorizonView v = view_of(h);
    if (h->durations.size() != (size_t)h->p.B * h->p.P * 4) v.durations = nullptr;
    if (h->win_start.empty()) v.win_start = nullptr;
    return v;
}

static ElemSide handle_side(hsddp_handle h, const int *idx)
{
    ElemSide s{};
    s.d = h->d; s.rec = nullptr; s.idx = idx;
    s.P = h->p.P; s.S = h->p.S; s.hcap = h->p.hcap; s.shared_refs = h->Bref == 1 ? 1 : 0;
    return s;
}

static ElemSide record_side(char *base, size_t S_cap)
{
    ElemSide s{};
    s.rec = base; s.idx = nullptr;
    s.P = HSDDP_MAX_PHASES; s.S = (int)S_cap; s.hcap = REC_HIST; s.shared_refs = 0;
    return s;
}

// the solver-info history with room for `need` entries per element, the rows held kept
static int grow_history(hsddp_handle h, int need)
{
    if (need <= h->p.hcap) return HSDDP_OK;
    const size_t B = h->p.B, old = h->p.hcap;
    float *nh = nullptr;
    if (hipMalloc(&nh, B * need * 4 * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HSDDP_ERR_ALLOC, "hipMalloc: the solver-info history");
    }
    HIPCHK(hipMemsetAsync(nh, 0, B * need * 4 * sizeof(float), h->stream));
    HIPCHK(hipMemcpy2DAsync(nh, (size_t)need * 16, h->hist, old * 16, old * 16, B, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    hipFree(h->hist);
    h->bytes += B * ((size_t)need - old) * 4 * sizeof(float);
    h->hist = nh;
    h->d.hist = nh;
    h->p.hcap = need;
    return HSDDP_OK;
}

// HSDDP_COPY_TIMING=1: the move kernels' device time (HIP events), summed over a call's launches
struct MoveTimer {
    bool on;
    hipStream_t st;
    float ms = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    MoveTimer(hipStream_t s) : st(s)
    {
        static const bool timing = std::getenv("HSDDP_COPY_TIMING") != nullptr;
        on = timing && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    }
    ~MoveTimer()
    {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
    void begin() { if (on) hipEventRecord(ev[0], st); }
    void end()  // (synchronises: a diagnostic)
    {
        if (!on) return;
        float t = 0;
        hipEventRecord(ev[1], st);
        if (hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) ms += t;
    }
};

// Where the moved elements come from: elements index[m] of a live handle, or host records [n].
struct MoveSource {
    hsddp_handle h;
    const int *index;
    const char *records;
};

// Slot dst_index[m] of dst becomes move m's source element.  Check, plan (plan_import_batch), the
// allocations, then apply and commit as hsddp_restart_elements does.  Order on the device: the
// sources that a same-handle move also overwrites are staged as records first (all of them when the
// strides change: the restride pass moves every row), records from the host are staged by their
// copy; then the restride pass, then the direct moves, then the staged ones.
static int move_elements(hsddp_handle dst, const MoveSource &src, int n, const int *dst_index, const char *who)
{
    if (!dst || (!src.h && !src.records) || n < 0) return fail(HSDDP_ERR_ARG, "null handle or records, or n < 0");
    if (n > 0 && (!dst_index || (src.h && !src.index))) return fail(HSDDP_ERR_ARG, "null index array");
    if (n == 0) return HSDDP_OK;  // nothing moves: nothing is launched, nothing changes
    Params &p = dst->p;
    const int B = p.B;
    const RecordLayout R = record_layout(p.Kc, dst->S_cap, p.fp32, true);
    int rc;
    // check: the two sides agree, both are settled, the indices
    const ElementKey kd = key_of(dst);
    if (src.h) {
        if (src.h->desc.device != dst->desc.device) return fail(HSDDP_ERR_ARG, "the two handles are on different devices");
        if ((rc = compatible(key_of(src.h), kd, false)) || (rc = settled(src.h, "source"))) return rc;
    }
    if ((rc = settled(dst, "destination"))) return rc;
    std::vector<ElementImport> in(n);
    std::vector<PhaseOverrides> ov(n);
    bool at_init = true;
    int hist_need = 0;
    if (src.h) {
        const HorizonView vs = element_view(src.h);
        for (int m = 0; m < n; ++m) {
            if (src.index[m] < 0 || src.index[m] >= vs.B) return fail(HSDDP_ERR_ARG, "source element index out of range");
            export_element(vs, src.index[m], in[m]);
            export_overrides(vs, src.index[m], ov[m]);
        }
        at_init = src.h->reb_at_init;
        hist_need = src.h->p.hcap;  // (room for whatever a source element holds)
    } else {
        for (int m = 0; m < n; ++m) {
            RecordHeader hd;
            std::memcpy(&hd, src.records + (size_t)m * R.bytes, sizeof hd);
            if (hd.version != RECORD_VERSION) return fail(HSDDP_ERR_ARG, "not an element record of this version");
            if ((rc = compatible(hd.key, kd, true))) return rc;
            if (hd.hist_n < 0 || hd.hist_n > REC_HIST) return fail(HSDDP_ERR_ARG, "damaged element record");
            in[m] = hd.host;
            std::memcpy(&ov[m], src.records + (size_t)m * R.bytes + R.pw, sizeof ov[m]);
            at_init = at_init && hd.reb_at_init != 0;
            hist_need = std::max(hist_need, hd.hist_n);
        }
    }
    if (kd.has_table)
        for (int m = 0; m < n; ++m)
            if (in[m].win_start < 0 || in[m].win_start >= dst->ref_n) return fail(HSDDP_ERR_ARG, "an element's window start lies outside the table");
    if (dst->Bref == 1)
        return fail(HSDDP_ERR_UNSUPPORTED, "the destination has shared references: an element of its own needs per-element "
                                           "references (ref_per_element = 1)");
    // plan: what the arriving elements mean for the batch (strides, layouts, rows, pairs, clocks)
    const std::vector<int> list(dst_index, dst_index + n);
    RestartBatch r;
    std::string why;
    if ((rc = plan_import_batch(element_view(dst), list, in.data(), r, why))) return fail(rc, why);
    const bool restride = r.restride, in_place = r.in_place, same = src.h == dst;
    // an arriving element's terrain rows pass hsddp_set_terrain's checks (a record is outside input)
    bool brings_terrain = false;
    for (int m = 0; m < n; ++m) {
        if (!in[m].has_terrain) continue;
        brings_terrain = true;
        for (int i = 0; i < in[m].L.P; ++i) {
            const double mu = in[m].terrain[2 * i], ground = in[m].terrain[2 * i + 1];
            if (!std::isfinite(mu) || !std::isfinite(ground) || !(mu > 0))
                return fail(HSDDP_ERR_ARG, "an element's terrain rows hold a non-finite value or a friction coefficient <= 0");
        }
    }
    if (brings_terrain && (rc = ensure_terrain_table(dst))) return rc;
    // ... and its weight row hsddp_set_element_weights' check
    bool brings_weights = false;
    for (int m = 0; m < n; ++m) {
        if (!in[m].has_weights) continue;
        brings_weights = true;
        hsddp_hkd_weights w;
        std::memcpy(&w, in[m].weights, sizeof w);
        if (!weights_finite(w)) return fail(HSDDP_ERR_ARG, "an element's weight row holds a non-finite value");
    }
    if (brings_weights && (rc = ensure_weights_table(dst))) return rc;
    // ... and its phase overrides hsddp_set_phase_weights'
    bool brings_pw = false;
    for (int m = 0; m < n; ++m) {
        if (!ov[m].has) continue;
        brings_pw = true;
        for (int i = 0; i < in[m].L.P; ++i) {
            if (!ov[m].set[i]) continue;
            hsddp_hkd_weights w;
            std::memcpy(&w, &ov[m].rows[(size_t)i * NW], sizeof w);
            if (!weights_finite(w)) return fail(HSDDP_ERR_ARG, "an element's phase weight rows hold a non-finite value");
        }
    }
    if (brings_pw && (rc = ensure_phase_weights_table(dst))) return rc;
    if (restride && !kd.has_table)
        return fail(HSDDP_ERR_UNSUPPORTED, "the move changes the destination's strides: its other elements' references "
                                           "are rebuilt from the table, and it has none");
    // the moves: staged (through records) or direct
    std::vector<int> direct, staged;
    {
        std::vector<char> is_dst(same ? B : 0, 0);
        if (same)
            for (int b : list) is_dst[b] = 1;
        for (int m = 0; m < n; ++m)
            ((!src.h || (same && (restride || is_dst[src.index[m]]))) ? staged : direct).push_back(m);
    }
    const int nd = (int)direct.size(), ns = (int)staged.size();
    // allocations: the history's room, the workspace (lists, layout records, staged records)
    HIPCHK(hipSetDevice(dst->desc.device));
    if (src.h && !same) HIPCHK(hipStreamSynchronize(src.h->stream));
    HIPCHK(hipStreamSynchronize(dst->stream));
    constexpr size_t LW = sizeof(Layout) / sizeof(int);
    const size_t ni = (size_t)2 * n + (in_place ? (size_t)n * LW : 0), ib = (ni * sizeof(int) + 255) & ~(size_t)255;
    const size_t wbytes = ib + (size_t)ns * R.bytes;
    char *buf = nullptr, *temp = nullptr;
    if (restride) {  // (the restride pass and its references use the handle's scratch)
        if (hipMalloc((void **)&temp, wbytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(HSDDP_ERR_ALLOC, "hipMalloc: the move's workspace");
        }
        buf = temp;
    } else if ((rc = scratch(dst, wbytes, &buf)))
        return rc;
    struct Release {
        char *p;
        ~Release() { if (p) hipFree(p); }
    } release{temp};
    if ((rc = grow_history(dst, hist_need))) return rc;
    // lists in move order direct, then staged: destination slot, source element, layout record
    std::vector<int> host(ni);
    int *hd_ = host.data(), *hs_ = hd_ + n;
    Layout *hl = (Layout *)(hs_ + n);
    for (int j = 0; j < n; ++j) {
        const int m = j < nd ? direct[j] : staged[j - nd];
        hd_[j] = list[m];
        hs_[j] = src.h ? src.index[m] : 0;
        if (in_place) hl[j] = in[m].L;
    }
    int *dd = (int *)buf, *dsrc = dd + n;
    const Layout *dl = in_place ? (const Layout *)(dsrc + n) : nullptr;
    char *stage = buf + ib;
    if ((rc = h2d(dd, host.data(), ni * sizeof(int), dst->stream))) return rc;
    MoveArgs a{};
    a.Kc = p.Kc; a.fp32 = p.fp32; a.R = R;
    MoveTimer timer(dst->stream);
    // apply: the staged sources first
    if (!src.h) {
        for (int j = 0; j < ns; ++j)
            if ((rc = h2d(stage + (size_t)j * R.bytes, src.records + (size_t)staged[j] * R.bytes, R.bytes, dst->stream))) return rc;
    } else if (ns) {
        a.n = ns; a.lay = nullptr;
        timer.begin();
        launch_move(a, handle_side(dst, dsrc + nd), record_side(stage, dst->S_cap), dst->stream);
        HIPCHK(hipGetLastError());
        timer.end();
    }
    std::vector<double> th;  // (read by its copy until the call's last synchronisation)
    if (restride) {  // the other elements' rows to the new strides (installs per-element layouts)
        // ... with the stored foot heights [B][P][4], which the shift leaves to the next rollout
        const size_t Po = p.P;
        std::vector<double> th_old((size_t)B * Po * 4);
        if ((rc = d2h(th_old.data(), dst->d.term_h, th_old.size() * sizeof(double)))) return rc;
        if ((rc = shift_apply(dst, r.stride_plan, false, nullptr, false))) return rc;
        dst->need_inputs = false;
        const size_t Pn = p.P;
        th.assign((size_t)B * Pn * 4, 0.0);
        for (size_t b = 0; b < (size_t)B; ++b)
            std::copy_n(&th_old[b * Po * 4], std::min(Po, Pn) * 4, &th[b * Pn * 4]);
        if ((rc = h2d(dst->d.term_h, th.data(), th.size() * sizeof(double), dst->stream))) return rc;
    }
    if (r.one) {
        adopt_shared_layout(dst, r.plans[0].L, &r.reach_in[0]);
    } else if (in_place) {
        for (int m = 0; m < n; ++m) {  // (the device records go with the move's kernel)
            dst->lays[list[m]] = r.plans[m].L;
            std::copy_n(&r.reach_in[(size_t)m * HSDDP_MAX_PHASES], HSDDP_MAX_PHASES,
                        &dst->reach_el[(size_t)list[m] * HSDDP_MAX_PHASES]);
        }
        if ((rc = repair_pairs(dst, list))) return rc;
    } else if (!restride) {
        if ((rc = set_layouts(dst, r.lays))) return rc;
        dst->reach_el.swap(r.reach);
    }
    // contact rows [B][P + 1][4] and durations [B][P][4]; at a new stride the others' rows have moved
    if (restride) {
        dst->contacts.swap(r.contacts);
        dst->durations.swap(r.durations);
        if ((rc = h2d((void *)dst->d.contacts, dst->contacts.data(), dst->contacts.size() * sizeof(int), dst->stream))) return rc;
    } else {
        const bool dur = dst->durations.size() == (size_t)B * p.P * 4;
        for (int m = 0; m < n; ++m) {
            int *c = &dst->contacts[(size_t)list[m] * (p.P + 1) * 4];
            std::fill_n(c, (p.P + 1) * 4, 0);
            std::copy_n(r.plans[m].contacts, (r.plans[m].L.P + 1) * 4, c);
            if (!dur) continue;
            double *q = &dst->durations[(size_t)list[m] * p.P * 4];
            std::fill_n(q, p.P * 4, 0.0);
            std::copy_n(r.plans[m].durations, r.plans[m].L.P * 4, q);
        }
    }
    dst->contacts_current = true;
    // the terrain rows arrive with the elements (a source without terrain: cparams rows); a
    // destination without terrain takes it up when an element brings some
    {
        const HorizonView v = view_of(dst);
        if (brings_terrain && dst->terrain.empty()) {
            dst->terrain.resize((size_t)B * p.P * 2);
            for (int b = 0; b < B; ++b) put_terrain_rows(nullptr, 0, p.P, v.fill, &dst->terrain[(size_t)b * p.P * 2]);
        }
        if (!dst->terrain.empty()) {
            for (int m = 0; m < n; ++m)
                put_terrain_rows(in[m].has_terrain ? in[m].terrain : nullptr, in[m].L.P, p.P, v.fill,
                                 &dst->terrain[(size_t)list[m] * p.P * 2]);
            dst->terrain_stale = true;
        }
    }
    // the weight rows arrive with the robots (from a handle with the table off: that handle's weights,
    // which are the destination's — compatible()); a destination with the table off turns it on when a
    // robot brings a row, its residents reading its desc.weights
    if (brings_weights && dst->weights.empty()) dst->weights.assign((size_t)B, dst->desc.weights);
    if (!dst->weights.empty()) {
        for (int m = 0; m < n; ++m) {
            if (in[m].has_weights) std::memcpy(&dst->weights[list[m]], in[m].weights, sizeof(hsddp_hkd_weights));
            else dst->weights[list[m]] = dst->desc.weights;
        }
        dst->weights_stale = true;
        dst->pw_stale = true;
    }
    // the phase overrides arrive with the robot's phases; a destination without any takes them up
    if (brings_pw || !dst->pw_set.empty()) {
        if (dst->pw_set.empty()) {
            dst->pw_set.assign((size_t)B * p.P, 0);
            dst->pw.assign((size_t)B * p.P * NW, 0.0);
        }
        for (int m = 0; m < n; ++m)
            put_phase_weight_rows(ov[m].has ? ov[m].set : nullptr, ov[m].rows, in[m].L.P, p.P, &dst->pw_set[(size_t)list[m] * p.P],
                                  &dst->pw[(size_t)list[m] * p.P * NW]);
        settle_phase_weights(dst);
    }
    // the windows (at a new stride every element's references are rebuilt; the arriving elements'
    // rows then replace theirs) and the clocks
    if (!r.win_start.empty()) dst->win_start = r.win_start;
    if (restride && (rc = build_refs(dst, dst->win_start.data(), dst->win_len, nullptr, dst->dt_sim, false))) return rc;
    dst->t_cur = r.t_cur;
    dst->t_el.swap(r.t_el);
    // the rows: the direct moves, then the staged ones
    timer.begin();
    if (nd) {
        a.n = nd; a.lay = dl;
        launch_move(a, handle_side(src.h, dsrc), handle_side(dst, dd), dst->stream);
    }
    if (ns) {
        a.n = ns; a.lay = dl ? dl + nd : nullptr;
        launch_move(a, record_side(stage, dst->S_cap), handle_side(dst, dd + nd), dst->stream);
    }
    HIPCHK(hipGetLastError());
    timer.end();
    HIPCHK(hipStreamSynchronize(dst->stream));  // (the pageable host rows above are read until here)
    if (timer.on)
        std::fprintf(stderr, "%s kernels ms: %.4f (B %d, moved %d%s%s)\n", who, timer.ms, B, n,
                     in_place ? ", in place" : restride ? ", new strides" : "", ns && src.h ? ", staged" : "");
    // what the handle caches of rows and layouts (as a restart leaves it); the ReB rows may now differ
    // from the initial pair
    dst->slots_fresh = false;
    dst->sim_fresh = false;
    dst->meas_held = false;
    if (!at_init) {
        dst->reb_at_init = false;
        p.reb_uniform = 0;
    }
    return HSDDP_OK;
}

extern "C" int hsddp_copy_elements(hsddp_handle dst, hsddp_handle src, int n, const int *dst_index, const int *src_index)
{
    if (!dst || !src) return fail(HSDDP_ERR_ARG, "null handle");
    return move_elements(dst, MoveSource{src, src_index, nullptr}, n, dst_index, "hsddp_copy_elements");
}

extern "C" size_t hsddp_element_record_bytes(const struct hsddp_handle_t *h)
{
    if (!h) { fail(HSDDP_ERR_ARG, "null handle"); return 0; }
    return record_layout(h->p.Kc, h->S_cap, h->p.fp32, true).bytes;
}

extern "C" int hsddp_export_elements(hsddp_handle h, int n, const int *index, void *records)
{
    if (!h || n < 0 || (n > 0 && (!index || !records))) return fail(HSDDP_ERR_ARG, "null argument");
    if (n == 0) return HSDDP_OK;
    int rc;
    if ((rc = settled(h, "source"))) return rc;
    const Params &p = h->p;
    for (int m = 0; m < n; ++m)
        if (index[m] < 0 || index[m] >= p.B) return fail(HSDDP_ERR_ARG, "element index out of range");
    const RecordLayout R = record_layout(p.Kc, h->S_cap, p.fp32, true);
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t ib = ((size_t)n * sizeof(int) + 255) & ~(size_t)255;
    char *buf;
    if ((rc = scratch(h, ib + (size_t)n * R.bytes, &buf))) return rc;
    if ((rc = h2d(buf, index, (size_t)n * sizeof(int), h->stream))) return rc;
    HIPCHK(hipMemsetAsync(buf + ib, 0, (size_t)n * R.bytes, h->stream));  // (rows past the strides: zero)
    MoveArgs a{};
    a.n = n; a.Kc = p.Kc; a.fp32 = p.fp32; a.R = R; a.lay = nullptr;
    MoveTimer timer(h->stream);
    timer.begin();
    launch_move(a, handle_side(h, (const int *)buf), record_side(buf + ib, h->S_cap), h->stream);
    HIPCHK(hipGetLastError());
    timer.end();
    HIPCHK(hipMemcpyAsync(records, buf + ib, (size_t)n * R.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (timer.on) std::fprintf(stderr, "hsddp_export_elements kernels ms: %.4f (B %d, moved %d)\n", timer.ms, p.B, n);
    // the headers: version, compatibility key, host bookkeeping
    const HorizonView v = element_view(h);
    const ElementKey key = key_of(h);
    for (int m = 0; m < n; ++m) {
        char *rec = (char *)records + (size_t)m * R.bytes;
        RecordHeader hd;
        std::memset(&hd, 0, sizeof hd);
        hd.version = RECORD_VERSION;
        hd.key = key;
        export_element(v, index[m], hd.host);
        hd.reb_at_init = h->reb_at_init ? 1 : 0;
        ElemState E;
        std::memcpy(&E, rec + R.el, sizeof E);
        hd.hist_n = E.hist_n;
        std::memcpy(rec, &hd, sizeof hd);
        PhaseOverrides po;
        export_overrides(v, index[m], po);
        std::memcpy(rec + R.pw, &po, sizeof po);
        if (E.hist_n > REC_HIST) rc = HSDDP_ERR_UNSUPPORTED;
    }
    if (rc) return fail(rc, "an element holds more solver-info entries than a record has room for (256)");
    return HSDDP_OK;
}

extern "C" int hsddp_import_elements(hsddp_handle h, int n, const int *index, const void *records)
{
    if (!h || n < 0 || (n > 0 && (!records || !index))) return fail(HSDDP_ERR_ARG, "null argument");
    if (n == 0) return HSDDP_OK;
    return move_elements(h, MoveSource{nullptr, nullptr, (const char *)records}, n, index, "hsddp_import_elements");
}

extern "C" int hsddp_get_phase_info(hsddp_handle h, int *contacts, double *durations)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    const Params &p = h->p;
    if (contacts) std::copy(h->contacts.begin(), h->contacts.end(), contacts);
    if (durations) {
        if (h->durations.size() != (size_t)p.B * p.P * 4)
            return fail(HSDDP_ERR_ARG, "no phase durations (references not built from a table)");
        std::copy(h->durations.begin(), h->durations.end(), durations);
    }
    return HSDDP_OK;
}
