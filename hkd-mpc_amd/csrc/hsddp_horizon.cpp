// hsddp_horizon.cpp — the MPC caller's side of the C-ABI, around the solve: command extraction
// (HKDMPCSolver::update_foot_placement + publish_mpc_cmd), the receding-horizon shift
// (HKDProblem::update, HKDProblem.cpp:117-222; its bookkeeping is hsddp_phases.cpp), the reference
// table and the per-slot references built from it, hsddp_advance, which steps all of them from
// the table, and hsddp_restart_elements, which starts single elements again as new problems.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>

#include "hsddp_handle.h"
#include "hsddp_mpc.h"
#include "hsddp_restart.h"

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
namespace {
// the bookkeeping's outcome: per slot map the phases after the steps (PhaseStepper) and their
// layout, and the map of each element (elements with equal layout, reach flags and step flags
// share one)
struct ShiftPlan {
    std::vector<std::vector<ShiftPhase>> phs;
    std::vector<Layout> nl;
    std::vector<int> map_id;  // [B]
};
}  // namespace

// the key under which elements share a slot map: horizons, shooting states, reach flags, step flags
static std::vector<int> shift_key(const Layout &L, const int *reach, int n_steps, const int *cc)
{
    std::vector<int> key(L.N, L.N + L.P);
    key.push_back(-1);
    key.insert(key.end(), L.ss, L.ss + L.P);
    key.insert(key.end(), reach, reach + L.P);
    key.insert(key.end(), cc, cc + n_steps);
    return key;
}

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
    const std::vector<std::vector<ShiftPhase>> &phs = plan.phs;
    const std::vector<Layout> &nl = plan.nl;
    const std::vector<int> &map_id = plan.map_id;
    const int nk = (int)phs.size();
    int Snew = 0, Pnew = 0;
    for (const Layout &L : nl) {
        if (control_slots(L) != p.Kc || (size_t)L.S > h->S_cap)
            return fail(HSDDP_ERR_ARG, "shifted layout exceeds the handle's capacity");
        Snew = std::max(Snew, L.S);
        Pnew = std::max(Pnew, L.P);
    }
    // slot maps [nk][Snew] (padding rows: zero) and [nk][Kc]; constraint-parameter maps: ReB source
    // per control slot [nk][Kc], phase source and appended touchdown constraints [nk][16]
    std::vector<int> smap((size_t)nk * Snew, -1), cmap((size_t)nk * p.Kc), rmap((size_t)nk * p.Kc);
    std::vector<int> pmap((size_t)nk * HSDDP_MAX_PHASES, -1), nadd((size_t)nk * HSDDP_MAX_PHASES, 0);
    for (int q = 0; q < nk; ++q) {
        size_t s = 0, k = 0, r = 0;
        for (size_t i = 0; i < phs[q].size(); ++i) {
            const auto &f = phs[q][i];
            for (int v : f.xs) smap[(size_t)q * Snew + s++] = v;
            for (int v : f.us) cmap[(size_t)q * p.Kc + k++] = v;
            for (int v : f.rs) rmap[(size_t)q * p.Kc + r++] = v;
            pmap[(size_t)q * HSDDP_MAX_PHASES + i] = f.src;
            nadd[(size_t)q * HSDDP_MAX_PHASES + i] = f.add;
        }
    }
    HIPCHK(hipSetDevice(h->desc.device));
    Bufs &d = h->d;
    int rc;
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
        for (int i = 0; i < nl[0].P; ++i) reach[i] = phs[0][i].reach;
        adopt_shared_layout(h, nl[0], reach);
    } else {
        std::vector<Layout> lays(B);
        std::vector<int> reach(B * HSDDP_MAX_PHASES, 0);
        for (size_t b = 0; b < B; ++b) {
            lays[b] = nl[map_id[b]];
            for (int i = 0; i < lays[b].P; ++i) reach[b * HSDDP_MAX_PHASES + i] = phs[map_id[b]][i].reach;
        }
        if ((rc = set_layouts(h, lays))) return rc;
        h->reach_el = reach;
    }
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
    const size_t B = h->p.B;
    std::map<std::vector<int>, int> keys;
    ShiftPlan plan;
    plan.map_id.assign(B, 0);
    // the handle's shared layout shifted by one set of flags (hsddp_shift): one key for the batch
    // (a per-element key and map lookup cost ≈ 1 µs an element: 4 ms of host time at B = 4096)
    const size_t nkey = (h->lays.empty() && bstride == 0) ? std::min<size_t>(B, 1) : B;
    for (size_t b = 0; b < nkey; ++b) {
        const Layout L = layout_of(h, b);
        const int *flags = cc + b * bstride;
        std::vector<int> key = shift_key(L, reach_of(h, b), n_steps, flags);
        auto it = keys.find(key);
        if (it == keys.end()) {
            PhaseStepper st(L, reach_of(h, b));
            Layout Ln;
            std::string why;
            int rc = 0;
            for (int j = 0; j < n_steps && !rc; ++j)
                if (!(rc = st.drop_front("shift", why))) rc = st.extend_back(flags[j], "shift", why);
            if (rc || (rc = st.finish(Ln, why))) return fail(rc, why);
            it = keys.emplace(std::move(key), (int)plan.phs.size()).first;
            plan.phs.push_back(std::move(st.ph));
            plan.nl.push_back(Ln);
        }
        plan.map_id[b] = it->second;
    }
    if (plan.phs.size() > 1 && h->Bref == 1 && B > 1)  // checked before any device work: the handle stays usable
        return fail(HSDDP_ERR_ARG, "the elements' shifts diverge into per-element layouts, which need per-element "
                                   "references (ref_per_element = 1)");
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
    h->win_start.clear();
    return HSDDP_OK;
}

// the phases' start times on the float clock of HKDProblem::initialization (t += dt_sim per knot)
static std::vector<float> clock_starts(const Layout &L, float dt_sim)
{
    std::vector<float> start(L.P);
    float t = 0.0f;
    for (int i = 0; i < L.P; ++i) {
        start[i] = t;
        for (int k = 0; k < L.N[i]; ++k) t += dt_sim;
    }
    return start;
}

// the window sample of every state slot of layout L, S entries (padding slots repeat the last
// sample): slot times as the reference forms them, t_offset (float, phase start relative to the
// first phase) + k dt (double), passed on as float (SinglePhase.cpp:243-287; set_time_offset,
// HKDProblem.cpp:103,208), snapped to a sample (QuadReference.cpp:60-76)
static std::vector<int> slot_samples(const Layout &L, const std::vector<float> &start, float dt_sim, float dt_ref,
                                     int sz, int S)
{
    std::vector<int> row(S, 0);
    for (int i = 0; i < L.P; ++i)
        for (int k = 0; k <= L.N[i]; ++k) {
            const float t = (float)((double)start[i] + k * (double)dt_sim);
            row[L.s0[i] + k] = sample_at(t, dt_ref, sz);
        }
    for (int sl = L.S; sl < S; ++sl) row[sl] = row[L.S - 1];
    return row;
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
    // the phases' start times, per layout: the caller's, or the float clock's
    auto starts_of = [&](const Layout &L) {
        if (!phase_start_times) return clock_starts(L, dt_sim);
        std::vector<float> start(L.P);
        for (int i = 0; i < L.P; ++i) start[i] = phase_start_times[i] - phase_start_times[0];
        return start;
    };
    const int sz = window_len - 1;
    // one slot map per distinct layout ([n_maps][S], padding slots repeat the last sample)
    std::map<std::vector<int>, int> keys;
    std::vector<int> idx, map_id(elem ? p.B : 0);
    std::vector<std::vector<float>> map_starts;
    for (int b = 0; b < (elem ? p.B : 1); ++b) {
        const Layout L = layout_of(h, b);
        std::vector<int> key(L.N, L.N + L.P);
        auto it = keys.find(key);
        if (it == keys.end()) {
            const std::vector<float> start = starts_of(L);
            const std::vector<int> row = slot_samples(L, start, dt_sim, h->ref_dt, sz, p.S);
            it = keys.emplace(key, (int)map_starts.size()).first;
            idx.insert(idx.end(), row.begin(), row.end());
            map_starts.push_back(start);
        }
        if (elem) map_id[b] = it->second;
    }
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
        h->durations.assign((size_t)p.B * p.P * 4, 0.0);
        for (int b = 0; b < p.B; ++b) {
            const std::vector<float> &start = map_starts[elem ? map_id[b] : 0];
            for (int i = 0; i < (int)start.size(); ++i) {
                const int k = std::min(window_start[Br == 1 ? 0 : b] + sample_at(start[i], h->ref_dt, sz), h->ref_n - 1);
                for (int l = 0; l < 4; ++l) h->durations[((size_t)b * p.P + i) * 4 + l] = h->table_host[k].status_dur[l];
            }
        }
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
    const Params &p = h->p;
    const int B = p.B, Br = h->Bref, sz = h->win_len - 1;
    const bool elem = !h->lays.empty();
    const float dt = h->ref_dt, dts = h->dt_sim;
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
    auto leq = [](float a, float b) { return a < b || std::abs(a - b) <= 1e-6f; };
    int adv = 0;  // samples per simulation step
    for (int i = 1; leq(i * dt, dts); ++i) adv++;
    // QuadReference::step for every step: the window starts and the clock (shared by the batch, or
    // each element's own once hsddp_restart_elements has set some element's back to 0)
    const int P0 = p.P;  // stride of the current contact rows [B][P0 + 1][4] and durations [B][P0][4]
    std::vector<std::vector<int>> wsj(n_steps);  // window starts at each step
    std::vector<std::vector<float>> relj(n_steps);  // new_end - new_start at each step, per clock
    std::vector<int> ws(h->win_start);
    std::vector<float> t_cur(h->t_el.empty() ? std::vector<float>(1, h->t_cur) : h->t_el);
    for (int j = 0; j < n_steps; ++j) {
        for (int a = 0; a < adv; ++a) {
            for (float &t : t_cur) t += dt;
            for (int &w : ws) w++;
        }
        for (int &w : ws)
            if (w >= h->ref_n) return fail(HSDDP_ERR_ARG, "the reference window ran past the table");
        wsj[j] = ws;
        for (float t : t_cur) relj[j].push_back((t + plan_duration) - t);  // new_end_time - new_start_time
    }
    auto rel_at = [&](int b, int j) { return relj[j][relj[j].size() == 1 ? 0 : b]; };
    auto sample_w = [&](const std::vector<int> &w, int b, float t) -> const hsddp_quad_state & {
        const int k = w[Br == 1 ? 0 : b] + sample_at(t, dt, sz);
        return h->table_host[std::min(k, h->ref_n - 1)];
    };
    // a phase's sample: of an old phase its row of the handle's contacts / durations, of one these
    // steps start the table's at the horizon end of its first step
    auto phase_contact = [&](int b, const ShiftPhase &f) -> const int * {
        return f.src >= 0 ? &h->contacts[((size_t)b * (P0 + 1) + f.src) * 4] : sample_w(wsj[f.born], b, rel_at(b, f.born)).contact;
    };
    auto phase_duration = [&](int b, const ShiftPhase &f) -> const double * {
        return f.src >= 0 ? &h->durations[((size_t)b * P0 + f.src) * 4] : sample_w(wsj[f.born], b, rel_at(b, f.born)).status_dur;
    };
    // with the handle's shared layout and window, an element whose contact rows equal element 0's
    // steps exactly as element 0 does (the MPC batch of one gait): its bookkeeping is element 0's
    std::vector<int> rep(B);
    for (int b = 0; b < B; ++b) {
        const size_t n = (size_t)(P0 + 1) * 4;
        rep[b] = (b > 0 && !elem && Br == 1 &&
                  std::equal(h->contacts.begin() + (size_t)b * n, h->contacts.begin() + (size_t)(b + 1) * n, h->contacts.begin()))
                     ? 0 : b;
    }
    // HKDProblem::update's bookkeeping (HKDProblem.cpp:126-202) of every element over the steps
    // (PhaseStepper), the flag of each step read off the table: the contact at the new horizon end
    // against the last phase's.  Beside the phases: the step flags, where the next-contact row
    // comes from and the slot map (elements with equal layout, reach flags and step flags share one)
    struct Walk {
        std::vector<int> flags;
        int P_old = 0;                       // the element's phases before the steps
        int next_kind = 0, next_step = -1;  // row P: 0 old row, 1 contact at relj, 2 at plan + dt_mpc
        int map = 0;
    };
    std::vector<Walk> wk(B);
    ShiftPlan plan;
    std::map<std::vector<int>, int> keys;
    std::string why;
    int rc;
    for (int b = 0; b < B; ++b) {
        if (rep[b] != b) continue;
        Walk &W = wk[b];
        const Layout L = layout_of(h, b);
        PhaseStepper st(L, reach_of(h, b));
        W.P_old = L.P;
        W.flags.assign(n_steps, 0);
        for (int j = 0; j < n_steps; ++j) {
            if ((rc = st.drop_front("advance", why))) return fail(rc, why);
            const int *nc = sample_w(wsj[j], b, rel_at(b, j)).contact, *lc = phase_contact(b, st.ph.back());
            int cc = 0;
            for (int l = 0; l < 4; ++l) cc |= nc[l] != lc[l];
            if ((rc = st.extend_back(cc, "advance", why))) return fail(rc, why);
            // a new phase carries no terminal constraint (identity reset)
            if (st.ph.back().born == j) { W.next_kind = 1; W.next_step = j; }
            if (st.ph.back().reach) { W.next_kind = 2; W.next_step = j; }
            W.flags[j] = cc;
        }
        if (b > 0 && !elem && W.flags == wk[0].flags) continue;  // element 0's layout, reach flags and step flags: map 0
        std::vector<int> key = shift_key(L, reach_of(h, b), n_steps, W.flags.data());
        auto it = keys.find(key);
        if (it == keys.end()) {
            Layout Ln;
            if ((rc = st.finish(Ln, why))) return fail(rc, why);
            it = keys.emplace(std::move(key), (int)plan.phs.size()).first;
            plan.phs.push_back(std::move(st.ph));
            plan.nl.push_back(Ln);
        }
        W.map = it->second;
    }
    plan.map_id.resize(B);
    for (int b = 0; b < B; ++b) plan.map_id[b] = wk[rep[b]].map;
    stage(0);
    // the shift: one slot map for the batch when it agrees (the shared layout stays shared; deferred),
    // else the elements' own (per-element layouts, which need per-element references; a touchdown
    // overflow is reported after the rest of the step either way)
    const bool agree = !elem && plan.phs.size() == 1;
    if (!agree && B > 1 && Br == 1)
        return fail(HSDDP_ERR_UNSUPPORTED, "elements disagree on a contact change, which takes per-element layouts "
                                           "and per-element references (ref_per_element = 1)");
    h->sim_shifted += n_steps;  // (hsddp_update_problem_simulated compares it with the simulation's steps)
    if ((rc = shift_apply(h, plan, agree, &overflow))) return rc;
    stage(1);
    const int P = p.P;  // the new stride (the largest layout's with per-element layouts)
    std::vector<int> contacts((size_t)B * (P + 1) * 4, 0);
    std::vector<double> dur((size_t)B * P * 4, 0.0);
    for (int b = 0; b < B; ++b) {
        const Walk &W = wk[rep[b]];
        const std::vector<ShiftPhase> &ph = plan.phs[W.map];
        const int Pb = (int)ph.size();
        for (int i = 0; i < Pb; ++i) {
            const int *cv = phase_contact(b, ph[i]);
            const double *dv = phase_duration(b, ph[i]);
            for (int l = 0; l < 4; ++l) {
                contacts[((size_t)b * (P + 1) + i) * 4 + l] = cv[l];
                dur[((size_t)b * P + i) * 4 + l] = dv[l];
            }
        }
        for (int l = 0; l < 4; ++l)
            contacts[((size_t)b * (P + 1) + Pb) * 4 + l] =
                W.next_kind == 0 ? h->contacts[((size_t)b * (P0 + 1) + W.P_old) * 4 + l]
                : W.next_kind == 1 ? sample_w(wsj[W.next_step], b, rel_at(b, W.next_step)).contact[l]
                                   : sample_w(wsj[W.next_step], b, plan_duration + dt_mpc).contact[l];
    }
    stage(2);
    if ((rc = build_refs(h, ws.data(), h->win_len, nullptr, dts, false))) return rc;
    stage(3);
    if (x0) {
        if ((rc = hsddp_update_problem(h, contacts.data(), x0, nullptr, nullptr, nullptr))) return rc;
    } else {  // x0 follows from the new first phase's contact: hsddp_update_problem(h, NULL, x0, NULL...)
        h->contacts.swap(contacts);
        h->contacts_current = true;
    }
    h->durations.swap(dur);
    if (h->t_el.empty()) h->t_cur = t_cur[0];
    else h->t_el = t_cur;
    stage(4);
    if (timing)
        std::fprintf(stderr, "hsddp_advance us: bookkeeping %.1f shift %.1f contacts %.1f refs %.1f update %.1f\n",
                     tstage[0], tstage[1], tstage[2], tstage[3], tstage[4]);
    if (contact_change)  // per step: some element saw a contact change (the batch's flag when it agrees)
        for (int j = 0; j < n_steps; ++j) {
            int f = 0;
            for (int b = 0; b < B; ++b) f |= wk[rep[b]].flags[j];
            contact_change[j] = f;
        }
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
    std::vector<int> &pr = h->pairs_host, &of = h->pair_of;
    int np = h->p.n_pairs;
    std::vector<int> freed, touched;
    for (int b : list) {
        const int q = of[b], partner = pr[2 * q] == b ? pr[2 * q + 1] : pr[2 * q];
        pr[2 * q] = partner;
        pr[2 * q + 1] = -1;
        if (partner < 0) freed.push_back(q);
        else touched.push_back(q);
        of[b] = -1;
    }
    std::map<std::vector<int>, std::vector<int>> groups;
    for (int b : list) {
        const Layout &L = h->lays[b];
        std::vector<int> key(L.N, L.N + L.P);
        key.push_back(-1);
        key.insert(key.end(), L.ss, L.ss + L.P);
        groups[key].push_back(b);
    }
    for (auto &g : groups)
        for (size_t j = 0; j < g.second.size(); j += 2) {
            int q;
            if (!freed.empty()) { q = freed.back(); freed.pop_back(); }
            else q = np++;
            if ((size_t)2 * q + 1 >= pr.size()) pr.resize((size_t)2 * q + 2, -1);
            pr[2 * q] = g.second[j];
            pr[2 * q + 1] = j + 1 < g.second.size() ? g.second[j + 1] : -1;
            of[pr[2 * q]] = q;
            if (pr[2 * q + 1] >= 0) of[pr[2 * q + 1]] = q;
            touched.push_back(q);
        }
    std::sort(freed.begin(), freed.end(), std::greater<int>());
    for (int q : freed) {  // emptied entries: the last pair moves in
        const int last = np - 1;
        if (q != last) {
            pr[2 * q] = pr[2 * last];
            pr[2 * q + 1] = pr[2 * last + 1];
            of[pr[2 * q]] = q;
            if (pr[2 * q + 1] >= 0) of[pr[2 * q + 1]] = q;
            touched.push_back(q);
        }
        --np;
    }
    if ((size_t)np > (size_t)h->p.B) return fail(HSDDP_ERR_ARG, "sweep pairs exceed the batch");
    int rc;
    for (int q : touched)
        if (q < np && (rc = h2d((int *)h->d.pairs + 2 * q, &pr[2 * q], 2 * sizeof(int), h->stream))) return rc;
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
    std::vector<int> list;
    for (int b = 0; b < B; ++b)
        if (mask[b]) list.push_back(b);
    const int n = (int)list.size();
    if (n == 0) return HSDDP_OK;  // nothing restarts: nothing is launched, nothing changes
    const bool all = n == B;
    if (!all && Br == 1)
        return fail(HSDDP_ERR_UNSUPPORTED, "shared references: a restart of some elements needs per-element references "
                                           "(ref_per_element = 1)");
    if (!h->refs_on_device || !h->contacts_current || h->contacts.size() != (size_t)B * (p.P + 1) * 4 ||
        h->durations.size() != (size_t)B * p.P * 4)
        return fail(HSDDP_ERR_ARG, "no references and contacts of the current layout on the handle (after hsddp_shift: "
                                   "hsddp_build_references and hsddp_update_problem first)");
    std::vector<RestartPlan> plans(n);
    std::string why;
    for (int m = 0; m < n; ++m) {
        if (Br == 1 && window_start[list[m]] != window_start[0])
            return fail(HSDDP_ERR_UNSUPPORTED, "shared references hold one window: every window start must be the same");
        if (int rc = plan_restart(h->table_host.data(), h->ref_n, window_start[list[m]], h->win_len, h->ref_dt,
                                  plan_duration, h->dt_sim, dt_mpc, p.Kc, plans[m], why))
            return fail(rc, why);
    }
    // The batch's largest P and S after the restart (the strides of the per-phase and per-slot
    // buffers).  Unlisted elements keep theirs, so the old strides stand unless a new layout exceeds
    // them or a listed element alone held them; only then is every element looked at.
    const bool elem = !h->lays.empty();
    int Pn = 0, Sn = 0;
    bool held = false;  // a listed element's old layout has the batch's largest P or S
    for (int m = 0; m < n; ++m) {
        Pn = std::max(Pn, plans[m].L.P);
        Sn = std::max(Sn, plans[m].L.S);
        const Layout &Lo = layout_of(h, list[m]);
        held = held || Lo.P == p.P || Lo.S == p.S;
    }
    if (!all) {
        if (!elem || !held || (Pn >= p.P && Sn >= p.S)) {
            Pn = std::max(Pn, p.P);
            Sn = std::max(Sn, p.S);
        } else {
            std::vector<char> listed(B, 0);
            for (int b : list) listed[b] = 1;
            for (int b = 0; b < B; ++b)
                if (!listed[b]) {
                    Pn = std::max(Pn, h->lays[b].P);
                    Sn = std::max(Sn, h->lays[b].S);
                }
        }
    }
    if ((size_t)Sn > h->S_cap) return fail(HSDDP_ERR_ARG, "restarted layout exceeds the handle's capacity");
    // one layout for the batch stays (or becomes) the handle's shared one: every element restarted
    // onto one layout, or some elements of a shared-layout handle restarted onto that layout with no
    // phase of it at its end.  (Elements of a per-element handle that come to agree stay per element.)
    bool one = true;
    for (int m = 1; m < n && one; ++m) one = !std::memcmp(&plans[m].L, &plans[0].L, sizeof(Layout));
    if (!all)
        one = one && !elem && !std::memcmp(&plans[0].L, &h->shared, sizeof(Layout)) &&
              std::all_of(h->reach_end.begin(), h->reach_end.end(), [](int r) { return r == 0; });
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const bool restride = Pn != p.P || Sn != p.S;
    // in place: the strides stand and the handle has per-element layouts already, so the listed
    // elements' layout records, sweep pairs and table rows are patched and nothing of size B is built
    const bool in_place = elem && !restride && !all;
    const int P0 = p.P;
    int rc;
    std::vector<Layout> lays;
    std::vector<int> reach;
    if (!in_place && !one) {  // every element's layout and reach flags after the restart
        lays.resize(B);
        reach.assign((size_t)B * HSDDP_MAX_PHASES, 0);
        for (int b = 0; b < B; ++b) {
            lays[b] = layout_of(h, b);
            std::copy(reach_of(h, b), reach_of(h, b) + lays[b].P, &reach[(size_t)b * HSDDP_MAX_PHASES]);
        }
        for (int m = 0; m < n; ++m) {
            lays[list[m]] = plans[m].L;
            std::fill_n(&reach[(size_t)list[m] * HSDDP_MAX_PHASES], HSDDP_MAX_PHASES, 0);
        }
    }
    if (restride) {
        // the other elements' rows to the new strides: a shift of no steps (identity maps; the listed
        // elements' rows come out zero and are written below)
        ShiftPlan plan;
        plan.map_id.assign(B, 0);
        std::map<std::vector<int>, int> keys;
        std::vector<int> listed(B, -1);
        for (int m = 0; m < n; ++m) listed[list[m]] = m;
        for (int b = 0; b < B; ++b) {
            const Layout L = listed[b] >= 0 ? plans[listed[b]].L : layout_of(h, b);
            std::vector<int> key = listed[b] >= 0 ? std::vector<int>(L.N, L.N + L.P) : shift_key(L, reach_of(h, b), 0, nullptr);
            key.push_back(listed[b] >= 0 ? -2 : -3);
            auto it = keys.find(key);
            if (it == keys.end()) {
                std::vector<ShiftPhase> ph;
                if (listed[b] >= 0) {
                    for (int i = 0; i < L.P; ++i) {
                        ShiftPhase f;
                        f.N = L.N[i]; f.ss = L.ss[i]; f.reach = 0;
                        f.xs.assign(f.N + 1, -1); f.us.assign(f.N, -1); f.rs.assign(f.N, -1);
                        ph.push_back(f);
                    }
                } else {
                    ph = PhaseStepper(L, reach_of(h, b)).ph;
                }
                it = keys.emplace(std::move(key), (int)plan.phs.size()).first;
                plan.phs.push_back(std::move(ph));
                plan.nl.push_back(L);
            }
            plan.map_id[b] = it->second;
        }
        const bool pending = h->need_inputs;
        if ((rc = shift_apply(h, plan, false, nullptr, false))) return rc;
        h->need_inputs = pending;
    }
    // the layouts (a restriding shift_apply has installed the per-element ones)
    if (one) {
        const int none[HSDDP_MAX_PHASES] = {0};
        adopt_shared_layout(h, plans[0].L, none);
    } else if (in_place) {
        for (int m = 0; m < n; ++m) {  // (the device records go with the restart's kernel)
            h->lays[list[m]] = plans[m].L;
            std::fill_n(&h->reach_el[(size_t)list[m] * HSDDP_MAX_PHASES], HSDDP_MAX_PHASES, 0);
        }
        if ((rc = repair_pairs(h, list))) return rc;
    } else if (!restride) {
        if ((rc = set_layouts(h, lays))) return rc;
        h->reach_el = reach;
    }
    // contact rows [B][P + 1][4] and durations [B][P][4]: the listed elements' new; at a new stride
    // the others' rows move
    const int P = p.P;
    if (restride) {
        std::vector<int> contacts((size_t)B * (P + 1) * 4, 0);
        std::vector<double> dur((size_t)B * P * 4, 0.0);
        for (int b = 0; b < B; ++b) {
            const int Pb = std::min(layout_of(h, b).P, P0);
            std::copy_n(&h->contacts[(size_t)b * (P0 + 1) * 4], (Pb + 1) * 4, &contacts[(size_t)b * (P + 1) * 4]);
            std::copy_n(&h->durations[(size_t)b * P0 * 4], Pb * 4, &dur[(size_t)b * P * 4]);
        }
        h->contacts.swap(contacts);
        h->durations.swap(dur);
    }
    std::vector<int> rows((size_t)n * (P + 1) * 4, 0);  // the listed elements' rows, compacted
    for (int m = 0; m < n; ++m) {
        const int b = list[m], Pb = plans[m].L.P;
        std::fill_n(&h->contacts[(size_t)b * (P + 1) * 4], (P + 1) * 4, 0);
        std::fill_n(&h->durations[(size_t)b * P * 4], P * 4, 0.0);
        std::copy_n(plans[m].contacts, (Pb + 1) * 4, &h->contacts[(size_t)b * (P + 1) * 4]);
        std::copy_n(plans[m].durations, Pb * 4, &h->durations[(size_t)b * P * 4]);
        std::copy_n(plans[m].contacts, (Pb + 1) * 4, &rows[(size_t)m * (P + 1) * 4]);
    }
    h->contacts_current = true;
    if (restride && (rc = h2d((void *)h->d.contacts, h->contacts.data(), h->contacts.size() * sizeof(int), h->stream)))
        return rc;
    // the window starts; references: at a new stride every element's are rebuilt; shared ones (every
    // element restarts) are built as a whole; else the kernel forms the listed elements' own
    for (int m = 0; m < n; ++m) h->win_start[Br == 1 ? 0 : list[m]] = window_start[list[m]];
    if (restride || Br == 1) {
        const std::vector<int> ws(h->win_start);
        if ((rc = build_refs(h, ws.data(), h->win_len, nullptr, h->dt_sim, false))) return rc;
    }
    // the clocks: QuadReference's t_cur restarts for the listed elements
    if (all) {
        h->t_cur = 0;
        h->t_el.clear();
    } else {
        if (h->t_el.empty()) h->t_el.assign(B, h->t_cur);
        for (int b : list) h->t_el[b] = 0;
    }
    // the device rows: list, window starts, slot maps (one per distinct new layout), contact rows, x0
    const int sz = h->win_len - 1;
    std::map<std::vector<int>, int> maps;
    std::vector<int> idx, map_id(n), start(n);
    for (int m = 0; m < n; ++m) {
        const Layout &L = plans[m].L;
        std::vector<int> key(L.N, L.N + L.P);
        auto it = maps.find(key);
        if (it == maps.end()) {
            const std::vector<int> row = slot_samples(L, clock_starts(L, h->dt_sim), h->dt_sim, h->ref_dt, sz, p.S);
            it = maps.emplace(std::move(key), (int)maps.size()).first;
            idx.insert(idx.end(), row.begin(), row.end());
        }
        map_id[m] = it->second;
        start[m] = window_start[list[m]];
    }
    std::vector<Layout> recs;  // the listed elements' layout records (in place: written by the kernel)
    if (in_place)
        for (int m = 0; m < n; ++m) recs.push_back(plans[m].L);
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
