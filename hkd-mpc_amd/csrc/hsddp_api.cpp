// hsddp_api.cpp — C-ABI of the batched HS-DDP solver (include/hsddp.h): the error state, the handle
// and its device memory, options, phase layouts, uploads and downloads, and the model-primitive and
// device-memory wrappers.  The solve loop is hsddp_solve.cpp, the MPC caller's side (commands,
// shift, references, hsddp_advance) hsddp_horizon.cpp, the defaults and INFO loaders
// hsddp_settings.cpp.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hsddp_handle.h"
#include "hsddp_measure.h"
#include "hsddp_simulate.h"

using namespace hsddp;

static thread_local std::string g_err;

int hsddp::fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

extern "C" int hsddp_ref_fail(int code, const char *msg) { return fail(code, msg); }

extern "C" const char *hsddp_last_error(void) { return g_err.c_str(); }
extern "C" const char *hsddp_version(void) { return "hsddp-mi355x 0.1 (gfx950, fp64)"; }

// ---- handle ----------------------------------------------------------------------------------
static void fill_params(hsddp_handle h)
{
    h->slots_fresh = false;
    Params &p = h->p;
    const hsddp_problem_desc &ds = h->desc;
    const hsddp_options &o = h->opt;
    p.dt = ds.dt;
    p.dt_m = ds.dt / hkd::kMass;
    {
        const char *tr = std::getenv("HSDDP_TRACE");
        p.trace = (tr && tr[0] == '1') ? 1 : 0;
    }
    p.mu = ds.cparams.mu_fric;
    p.grf_delta = ds.cparams.grf_delta; p.grf_delta_min = ds.cparams.grf_delta_min; p.grf_eps = ds.cparams.grf_eps;
    p.td_sigma = ds.cparams.td_sigma; p.td_sigma_max = ds.cparams.td_sigma_max; p.td_lambda = ds.cparams.td_lambda;
    p.ground = ds.cparams.ground_height;
    const hsddp_hkd_weights &w = ds.weights;
    for (int j = 0; j < 3; ++j) { p.qbase[j] = w.q_eul[j]; p.qbase[3 + j] = w.q_pos[j]; p.qbase[6 + j] = w.q_omega[j]; p.qbase[9 + j] = w.q_v[j]; }
    p.q_qJ = w.q_qJ;
    for (int j = 0; j < 24; ++j) p.qf_scale[j] = w.qf_scale[j];
    p.qf_gain = w.qf_gain; p.r_grf = w.r_grf; p.r_qJd = w.r_qJd;
    for (int j = 0; j < 3; ++j) p.foot_w[j] = w.foot_w[j];
    p.foot_gain = w.foot_gain; p.foot_term_cost = w.foot_term_cost; p.foot_term_grad = w.foot_term_grad;
    p.alpha = o.alpha; p.gamma = o.gamma; p.update_penalty = o.update_penalty; p.update_relax = o.update_relax;
    p.update_regularization = o.update_regularization; p.update_ReB = o.update_ReB;
    p.cost_thresh = o.cost_thresh; p.tconstr_thresh = o.tconstr_thresh; p.pconstr_thresh = o.pconstr_thresh;
    p.feas_thresh = o.dynamics_feas_thresh; p.merit_scale = o.merit_scale; p.merit_offset = o.merit_offset;
    p.AL_active = o.AL_active; p.ReB_active = o.ReB_active; p.no_early_exit = o.no_early_exit;
    p.ms0 = o.MS ? 0 : 1;  // single shooting (MultiPhaseDDP.cpp:326-329; SinglePhase.cpp:214)
    // With update_ReB = update_relax = 1 (the shipped settings) update_REB_params leaves every
    // (delta, eps) at its initial value (ConstraintsBase.h:168-183): the kernels then read the two
    // scalars instead of the per-knot arrays.
    p.reb_uniform = o.update_ReB == 1.0 && o.update_relax == 1.0 && p.grf_delta >= p.grf_delta_min && h->reb_at_init;
    p.grf_inv_delta = 1.0 / p.grf_delta;
    p.grf_log_delta = std::log(p.grf_delta);
    // attempts of backward_sweep_regularized after the first, at most (from mu = 0: 1e-3, then
    // x update_regularization while <= 1e2); the parallel retry holds that many per deferred element
    int M = 0;
    if (o.update_regularization > 1) {
        double mu = 0;
        for (;;) {
            mu = std::fmax(mu * o.update_regularization, 1e-03);
            if (mu > 1e2) break;
            if (++M > 64) { M = 0; break; }
        }
    }
    p.retry_m = M;
    // value export writes G[0], H[0] from the sweep that succeeds: the in-kernel retry loop only.
    // Below 4 elements (C1: one robot) the retries run in k_riccati too: the retry and select
    // launches (≈ 10 µs of a 340 µs inner iteration at B = 1) cost more than the rare sequential
    // retry of a lone element saves.
    p.retry_cap = (M > 0 && M <= h->retry_m_alloc && !p.store_value && p.B >= 4) ? h->retry_cap_alloc : 0;
}

// the solver-info history holds every entry one solve with the handle's options can push: the
// initial one and one per inner iteration (MultiPhaseDDP.cpp:277-280, 368-371)
static int ensure_history(hsddp_handle h)
{
    // (with per-element budgets: the largest element's too)
    const long need = std::max(1 + (long)std::max(0, h->opt.max_AL_iter) * std::max(0, h->opt.max_DDP_iter),
                               h->budgets_on ? 1 + h->bud_hist : 0L);
    if (h->hist && need <= h->p.hcap) return HSDDP_OK;
    const int cap = (int)std::min<long>(std::max<long>(need, 16), 1 << 20);
    float *nh = nullptr;
    HIPCHK(hipMalloc(&nh, (size_t)h->p.B * cap * 4 * sizeof(float)));
    HIPCHK(hipMemset(nh, 0, (size_t)h->p.B * cap * 4 * sizeof(float)));
    HIPCHK(hipStreamSynchronize(nullptr));  // (null-stream work is not ordered with h->stream)
    if (h->hist) {
        HIPCHK(hipStreamSynchronize(h->stream));
        hipFree(h->hist);
        h->bytes -= (size_t)h->p.B * h->p.hcap * 4 * sizeof(float);
    }
    h->hist = nh;
    h->d.hist = nh;
    h->p.hcap = cap;
    h->bytes += (size_t)h->p.B * cap * 4 * sizeof(float);
    return HSDDP_OK;
}

extern "C" int hsddp_create(const hsddp_problem_desc *desc, hsddp_handle *out)
{
    if (!desc || !out) return fail(HSDDP_ERR_ARG, "null argument");
    if (desc->batch < 1 || desc->n_phases < 1 || desc->n_phases > HSDDP_MAX_PHASES || !(desc->dt > 0))
        return fail(HSDDP_ERR_ARG, "invalid batch / n_phases / dt");
    Layout L0;  // every knot a shooting state (HKDProblem.cpp:104)
    std::string why;
    if (int rc = build_layout(desc->n_phases, desc->horizons, nullptr, L0, why)) return fail(rc, why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(HSDDP_ERR_DEVICE, "no HIP device available (the solver has no CPU fallback)");
    if (desc->device < 0 || desc->device >= ndev) return fail(HSDDP_ERR_DEVICE, "device ordinal out of range");
    HIPCHK(hipSetDevice(desc->device));
    hsddp_handle h = new hsddp_handle_t();
    h->desc = *desc;
    hsddp_default_options(&h->opt);
    Params &p = h->p;
    p.B = desc->batch;
    p.Kc = control_slots(L0);
    p.ref_per_element = desc->ref_per_element ? 1 : 0;
    p.fp32 = desc->riccati_fp32 ? 1 : 0;
    h->Bref = p.ref_per_element ? p.B : 1;
    adopt_shared_layout(h, L0, nullptr);  // (no reach flags: HKDProblem.cpp:56-57 compares a contact with itself, quirk A15)
    fill_params(h);
    // State-slot buffers hold Kc + HSDDP_MAX_PHASES slots (a receding-horizon shift keeps Kc and can
    // add phases, S = Kc + P); per-phase buffers hold HSDDP_MAX_PHASES phases.
    h->S_cap = (size_t)p.Kc + HSDDP_MAX_PHASES;
    const size_t B = p.B, S = h->S_cap, Kc = p.Kc, P = HSDDP_MAX_PHASES, Br = h->Bref;
    Bufs &d = h->d;
    int *contacts; double *x0, *rx, *ru, *rf;
    int rc = 0;
    if ((rc = dalloc(h, contacts, B * (P + 1) * 4)) || (rc = dalloc(h, x0, B * NX)) || (rc = dalloc(h, rx, Br * S * NX)) ||
        (rc = dalloc(h, ru, Br * S * NX)) || (rc = dalloc(h, rf, Br * S * 12)) || (rc = dalloc(h, d.ref_t, REF_COLS * Br * S)) ||
        (rc = dalloc(h, d.X3, 3 * B * S * NX)) ||
        (rc = dalloc(h, d.D3, 3 * B * S * NX)) || (rc = dalloc(h, d.U3, 3 * B * Kc * NX)) || (rc = dalloc(h, d.sel, B)) ||
        (rc = dalloc(h, d.cf_u, B * Kc * 12)) || (rc = dalloc(h, d.cf_flag, B * Kc)) ||
        (rc = dalloc(h, d.dX, B * S * NX)) ||
        (rc = dalloc(h, d.dU, B * Kc * NX)) ||
        (rc = dalloc(h, d.du, B * Kc * NX)) || (rc = dalloc(h, d.dbg, B * 16)) ||
        (p.fp32 ? ((rc = dalloc(h, d.K32, B * Kc * KCW)) || (rc = dalloc(h, d.lq32, B * Kc * LQW32)) ||
                   (rc = dalloc(h, d.def32, B * S * NX)))
                : ((rc = dalloc(h, d.K, B * Kc * KCW)) || (rc = dalloc(h, d.lq, B * Kc * LQW)))) ||
        (rc = dalloc(h, d.term, B * P * TW)) || (rc = dalloc(h, d.reb_delta, B * Kc * 20)) ||
        (rc = dalloc(h, d.reb_eps, B * Kc * 20)) || (rc = dalloc(h, d.al_sigma, B * P * MTD * 4)) ||
        (rc = dalloc(h, d.al_lambda, B * P * MTD * 4)) || (rc = dalloc(h, d.td_mask, B * P * MTD)) ||
        (rc = dalloc(h, d.term_h, B * P * 4)) ||
        (rc = dalloc(h, d.slot_cost, B * S)) || (rc = dalloc(h, d.slot_feas, B * S)) || (rc = dalloc(h, d.slot_viol, B * S)) ||
        (rc = dalloc(h, d.slot_div, B * S)) || (rc = dalloc(h, d.el, B)) || (rc = dalloc(h, d.counter, 8)) || (rc = dalloc(h, d.ls_live, LS_LIVE)) ||
        (rc = dalloc(h, (Layout *&)d.lay, B)) || (rc = dalloc(h, (int *&)d.pairs, 2 * B + 2))) {
        hsddp_destroy(h);
        return rc;
    }
    d.contacts = contacts; d.x0 = x0; d.ref_x = rx; d.ref_u = ru; d.ref_foot = rf;
    d.ref_tw = Br * S;
    d.xs3 = B * S * NX;  // (S = S_cap here)
    d.us3 = B * Kc * NX;
    d.rows3 = (int)(B * S);
    d.urows3 = (int)(B * Kc);
    {   // parallel regularisation retries: p.retry_m attempts for each of up to `cap` deferred elements
        // per launch (HSDDP_SEQUENTIAL_RETRY=1 keeps every retry inside k_riccati: a diagnostic for
        // tests).  Scratch per deferred element: M attempts x (Kc gain rows + Kc dU rows), 8.5 MB at the
        // metric's horizon in fp64 (17 x 200 x 312 x 8 B).  The cap is 128 elements within a 256 MiB
        // budget (30 at the metric's horizon; device_bytes counts it): the oracle's jump solves defer a
        // few elements of 4096 per iteration, and deferrals past the cap run the same retries inside
        // k_riccati.  HSDDP_RETRY_CAP=n lowers the cap (a diagnostic: tests use it to send deferrals
        // past the cap into the in-kernel loop).
        const char *seq = std::getenv("HSDDP_SEQUENTIAL_RETRY");
        const char *capenv = std::getenv("HSDDP_RETRY_CAP");
        const size_t per_elem = (size_t)std::max(1, p.retry_m) * Kc * (KCW * (p.fp32 ? 4 : 8) + NX * 8 + 4);
        size_t cap = std::min<size_t>(std::min<size_t>(128, B), std::max<size_t>(2, ((size_t)256 << 20) / per_elem));
        if (capenv && std::atoi(capenv) > 0) cap = std::min<size_t>(cap, (size_t)std::atoi(capenv));
        const size_t M = (seq && seq[0] == '1') ? 0 : p.retry_m, n = cap * M;
        if (M > 0) {
            void *rk;
            if ((rc = dalloc(h, d.retry_list, cap)) || (rc = dalloc(h, d.retry_count, 1)) ||
                (rc = dalloc(h, d.retry_flag, n)) || (rc = dalloc(h, d.retry_dU, n * Kc * NX)) ||
                (rc = dalloc(h, d.retry_dv, n)) ||
                (rc = p.fp32 ? dalloc(h, (float *&)rk, n * Kc * KCW) : dalloc(h, (double *&)rk, n * Kc * KCW))) {
                hsddp_destroy(h);
                return rc;
            }
            d.retry_K = rk;
            h->retry_cap_alloc = (int)cap;
            h->retry_m_alloc = (int)M;
            fill_params(h);
        }
    }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&h->host_counter, 16 * sizeof(int), 0) != hipSuccess) {
        hsddp_destroy(h);
        return fail(HSDDP_ERR_DEVICE, "stream / pinned allocation failed");
    }
    if ((rc = ensure_history(h))) {
        hsddp_destroy(h);
        return rc;
    }
    launch_init_params(p, d, h->stream);
    launch_reset_elements(p, d, h->stream);
    if (hipStreamSynchronize(h->stream) != hipSuccess) {
        hsddp_destroy(h);
        return fail(HSDDP_ERR_DEVICE, "kernel launch failed at create (is the library built for this GPU?)");
    }
    *out = h;
    return HSDDP_OK;
}

extern "C" int hsddp_destroy(hsddp_handle h)
{
    if (!h) return HSDDP_OK;
    hipSetDevice(h->desc.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void *p : h->allocs) hipFree(p);
    if (h->scratch) hipFree(h->scratch);
    if (h->ref_table) hipFree(h->ref_table);
    if (h->hist) hipFree(h->hist);
    if (h->value0) hipFree(h->value0);
    if (h->sim_buf) hipFree(h->sim_buf);

    for (auto &g : h->iter_graph)
        if (g.exec) hipGraphExecDestroy(g.exec);
    for (hipEvent_t e : h->iter_done)
        if (e) hipEventDestroy(e);
    if (h->host_counter) hipHostFree(h->host_counter);
    if (h->terrain_pin) hipHostFree(h->terrain_pin);
    if (h->terrain_up) hipEventDestroy(h->terrain_up);
    if (h->weights_pin) hipHostFree(h->weights_pin);
    if (h->weights_up) hipEventDestroy(h->weights_up);
    if (h->pw_pin) hipHostFree(h->pw_pin);
    if (h->pw_up) hipEventDestroy(h->pw_up);
    if (h->copy_stream) hipStreamSynchronize(h->copy_stream);
    for (int q = 0; q < 2; ++q) {
        if (h->cmd_dev[q]) hipFree(h->cmd_dev[q]);
        if (h->cmd_host[q]) hipHostFree(h->cmd_host[q]);
        if (h->cmd_ready[q]) hipEventDestroy(h->cmd_ready[q]);
        if (h->cmd_copied[q]) hipEventDestroy(h->cmd_copied[q]);
        if (h->cmd_in_host[q]) hipHostFree(h->cmd_in_host[q]);
    }
    if (h->copy_stream) hipStreamDestroy(h->copy_stream);
    for (hipEvent_t e : h->events) hipEventDestroy(e);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return HSDDP_OK;
}

extern "C" int hsddp_validate_options(const hsddp_options *o)
{
    if (!o) return fail(HSDDP_ERR_ARG, "null argument");
    if (!(o->alpha > 0 && o->alpha < 1)) return fail(HSDDP_ERR_ARG, "alpha must lie in (0, 1)");
    if (o->max_AL_iter < 0 || o->max_DDP_iter < 0) return fail(HSDDP_ERR_ARG, "negative iteration budget");
    // backward_sweep_regularized (MultiPhaseDDP.cpp:150-167) raises mu = max(mu * factor, 1e-3)
    // until a sweep succeeds or mu > 1e2.  A factor <= 1 never gets there (the reference spins
    // forever on the first failed sweep) and a factor barely above 1 takes thousands of sweeps per
    // failure; both are refused rather than left to hang a GPU wave.
    if (!(o->update_regularization > 1))
        return fail(HSDDP_ERR_ARG, "update_regularization must exceed 1 (the regularisation schedule would never end)");
    int m = 0;
    for (double mu = 0;; ++m) {
        mu = std::fmax(mu * o->update_regularization, 1e-03);
        if (mu > 1e2) break;
        if (m >= HSDDP_MAX_REG_ATTEMPTS)
            return fail(HSDDP_ERR_ARG, "update_regularization too close to 1: more than HSDDP_MAX_REG_ATTEMPTS "
                                       "regularisation retries per failed sweep");
    }
    return HSDDP_OK;
}

extern "C" int hsddp_set_options(hsddp_handle h, const hsddp_options *o)
{
    if (!h || !o) return fail(HSDDP_ERR_ARG, "null argument");
    int rc = hsddp_validate_options(o);
    if (rc) return rc;
    // the solver-info history must hold every entry of the new budget (1 + outer x inner)
    if (1 + (long)std::max(0, o->max_AL_iter) * std::max(0, o->max_DDP_iter) > (1L << 20))
        return fail(HSDDP_ERR_ARG, "max_AL_iter * max_DDP_iter exceeds the solver-info history (2^20 entries)");
    const hsddp_options old = h->opt;
    h->opt = *o;
    if ((rc = ensure_history(h))) {  // allocation failed: the handle keeps its previous options
        h->opt = old;
        return rc;
    }
    fill_params(h);
    return HSDDP_OK;
}

// MultiPhaseDDP::solve's loop bounds (MultiPhaseDDP.cpp:257, 304) per element: the bounds go to the
// device array the decision kernels read (hsddp_internal.h); the host loops to the largest.
extern "C" int hsddp_set_element_budgets(hsddp_handle h, const int *max_AL_iter, const int *max_DDP_iter)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!max_AL_iter && !max_DDP_iter) {  // back to the handle-wide options
        h->budgets_on = false;
        return HSDDP_OK;
    }
    if (!max_AL_iter || !max_DDP_iter) return fail(HSDDP_ERR_ARG, "budgets: both arrays or neither");
    const int B = h->p.B;
    std::vector<int> bud((size_t)B * 2);
    int al = 0, ddp = 0;
    long hist = 0;
    for (int b = 0; b < B; ++b) {
        if (max_AL_iter[b] < 0 || max_DDP_iter[b] < 0) return fail(HSDDP_ERR_ARG, "negative iteration budget");
        if ((long)max_AL_iter[b] * max_DDP_iter[b] >= (1L << 20))
            return fail(HSDDP_ERR_ARG, "max_AL_iter * max_DDP_iter exceeds the solver-info history (2^20 entries)");
        bud[2 * b] = max_AL_iter[b];
        bud[2 * b + 1] = max_DDP_iter[b];
        al = std::max(al, max_AL_iter[b]);
        ddp = std::max(ddp, max_DDP_iter[b]);
        hist = std::max(hist, (long)max_AL_iter[b] * max_DDP_iter[b]);
    }
    HIPCHK(hipSetDevice(h->desc.device));
    int rc;
    if (!h->budgets) {
        if ((rc = dalloc(h, h->budgets, (size_t)B * 2))) {
            h->budgets = nullptr;
            (void)hipGetLastError();
            return rc;
        }
    }
    const bool was = h->budgets_on;
    const long hist_was = h->bud_hist;
    h->budgets_on = true;
    h->bud_hist = hist;
    if ((rc = ensure_history(h))) {  // allocation failed: the handle keeps what it had
        h->budgets_on = was;
        h->bud_hist = hist_was;
        return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->budgets, bud.data(), bud.size() * sizeof(int), hipMemcpyHostToDevice));
    h->bud_AL = al;
    h->bud_DDP = ddp;
    return HSDDP_OK;
}

void hsddp::adopt_shared_layout(hsddp_handle h, const Layout &L, const int *reach)
{
    Params &p = h->p;
    h->shared = L;
    p.P = L.P;
    p.S = L.S;
    p.has_tail = L.has_tail;
    p.elem_layout = 0;
    for (int i = 0; i < HSDDP_MAX_PHASES; ++i) {  // (L's entries past P are zero)
        p.N[i] = L.N[i]; p.s0[i] = L.s0[i]; p.k0[i] = L.k0[i]; p.ss[i] = L.ss[i];
        h->desc.horizons[i] = L.N[i];
    }
    h->desc.n_phases = L.P;
    h->lays.clear();
    h->reach_el.clear();
    h->reach_end.assign(L.P, 0);
    if (reach) h->reach_end.assign(reach, reach + L.P);
}

int hsddp::set_layouts(hsddp_handle h, const std::vector<Layout> &lays)
{
    h->slots_fresh = false;
    Params &p = h->p;
    const int B = p.B;
    int Pmax = 0, Smax = 0, tail = 0;
    for (auto &L : lays) { Pmax = std::max(Pmax, L.P); Smax = std::max(Smax, L.S); tail |= L.has_tail; }
    std::vector<int> pairs = pair_layouts(lays);  // (patched in place by hsddp_restart_elements: patch_pairs)
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipMemcpy((void *)h->d.lay, lays.data(), B * sizeof(Layout), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((void *)h->d.pairs, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice));
    h->lays = lays;
    h->pair_of.assign(B, -1);
    for (size_t q = 0; q < pairs.size(); ++q)
        if (pairs[q] >= 0) h->pair_of[pairs[q]] = (int)(q / 2);
    h->pairs_host.swap(pairs);
    p.elem_layout = 1;
    p.n_pairs = (int)h->pairs_host.size() / 2;
    p.P = Pmax;  // strides of the per-phase and per-slot buffers
    p.S = Smax;
    p.has_tail = tail;
    for (int i = 0; i < HSDDP_MAX_PHASES; ++i) { p.N[i] = 0; p.s0[i] = 0; p.k0[i] = 0; p.ss[i] = 0; }
    return HSDDP_OK;
}

extern "C" int hsddp_set_element_layouts(hsddp_handle h, const int *n_phases, const int *horizons)
{
    if (!h || !n_phases || !horizons) return fail(HSDDP_ERR_ARG, "null argument");
    Params &p = h->p;
    const int B = p.B;
    if (B > 1 && h->Bref == 1)  // a shared reference is laid out for one layout
        return fail(HSDDP_ERR_ARG, "per-element layouts need per-element references (ref_per_element = 1)");
    std::vector<Layout> lays(B);
    std::string why;
    int rc;
    for (int b = 0; b < B; ++b) {
        Layout &L = lays[b];
        const int P = n_phases[b];
        if (P < 1 || P > HSDDP_MAX_PHASES) return fail(HSDDP_ERR_ARG, "element n_phases must lie in 1..16");
        if ((rc = build_layout(P, horizons + (size_t)b * HSDDP_MAX_PHASES, nullptr, L, why))) return fail(rc, why);
        if (control_slots(L) != p.Kc) return fail(HSDDP_ERR_ARG, "every element's horizons must sum to the handle's Kc");
    }
    if ((rc = set_layouts(h, lays))) return rc;
    h->reach_el.assign((size_t)B * HSDDP_MAX_PHASES, 0);  // HKDProblem.cpp:56-57 (quirk A15)
    h->terrain.clear();       // (the phases it described are gone)
    drop_phase_weights(h);    // (and the cost objects the overrides belonged to)
    h->have_problem = false;  // inputs of the new layouts next (hsddp_upload_problem)
    h->sim_fresh = false;
    h->contacts_current = false;
    h->refs_on_device = false;
    h->ref_cols_stale = true;
    return HSDDP_OK;
}

// the layout of every element: n_phases [B], horizons / shooting / reach_end [B][16] (any NULL)
extern "C" int hsddp_get_element_layouts(hsddp_handle h, int *n_phases, int *horizons, int *shooting, int *reach_end)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    for (size_t b = 0; b < (size_t)h->p.B; ++b) {
        const Layout L = layout_of(h, b);
        if (n_phases) n_phases[b] = L.P;
        for (int i = 0; i < HSDDP_MAX_PHASES; ++i) {
            const bool in = i < L.P;
            if (horizons) horizons[b * HSDDP_MAX_PHASES + i] = in ? L.N[i] : 0;
            if (shooting) shooting[b * HSDDP_MAX_PHASES + i] = in ? L.ss[i] : 0;
            if (reach_end) reach_end[b * HSDDP_MAX_PHASES + i] = in ? reach_of(h, b)[i] : 0;
        }
    }
    return HSDDP_OK;
}

extern "C" int hsddp_get_strides(hsddp_handle h, int *n_phases, int *state_slots)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (n_phases) *n_phases = h->p.P;
    if (state_slots) *state_slots = h->p.S;
    return HSDDP_OK;
}

extern "C" int hsddp_get_layout(hsddp_handle h, int *n_phases, int *horizons, int *shooting, int *reach_end)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->lays.empty()) return fail(HSDDP_ERR_UNSUPPORTED, "per-element layouts: hsddp_get_element_layouts");
    const Params &p = h->p;
    if (n_phases) *n_phases = p.P;
    for (int i = 0; i < p.P; ++i) {
        if (horizons) horizons[i] = p.N[i];
        if (shooting) shooting[i] = p.ss[i];
        if (reach_end) reach_end[i] = h->reach_end[i];
    }
    return HSDDP_OK;
}

// The caller's own receding-horizon bookkeeping applied to a live handle (the C++ facade's
// MultiPhaseDDP after HKDProblem::update, HKDProblem.cpp:117-222): a new shared layout of the same
// Kc, with each phase's shooting states SS_set = {0 .. shooting[i] - 1} (SinglePhase.h:161-164).
// Host only; the inputs and warm start of the new layout are uploaded next.
extern "C" int hsddp_set_layout(hsddp_handle h, int n_phases, const int *horizons, const int *shooting,
                                const int *reach_end)
{
    if (!h || !horizons) return fail(HSDDP_ERR_ARG, "null argument");
    Layout L;
    std::string why;
    if (int rc = build_layout(n_phases, horizons, shooting, L, why)) return fail(rc, why);
    if (control_slots(L) != h->p.Kc) return fail(HSDDP_ERR_ARG, "the layout's horizons must sum to the handle's Kc");
    if ((size_t)L.S > h->S_cap) return fail(HSDDP_ERR_ARG, "layout exceeds the handle's state-slot capacity");
    h->slots_fresh = false;
    int reach[HSDDP_MAX_PHASES];
    for (int i = 0; i < n_phases; ++i) reach[i] = reach_end && reach_end[i] ? 1 : 0;
    adopt_shared_layout(h, L, reach);
    h->terrain.clear();       // (the phases it described are gone)
    drop_phase_weights(h);    // (and the cost objects the overrides belonged to)
    h->have_problem = false;  // inputs of the new layout next (hsddp_upload_problem)
    h->sim_fresh = false;
    h->need_inputs = false;
    h->contacts_current = false;
    h->refs_on_device = false;
    h->ref_cols_stale = true;
    return HSDDP_OK;
}

// hsddp_update_problem_measured's records: [B] on the host (on_device = 0) or on the handle's device
struct Measured {
    const hsddp_robot_state *states;
    int on_device;
};

// a buffer of the measured-state ingest, allocated at its first use: counted by hsddp_device_bytes
// and freed with the handle; a failed allocation leaves the handle as it was
template <typename T>
static int measured_alloc(hsddp_handle h, T *&ptr, size_t n)
{
    if (ptr) return HSDDP_OK;
    const int rc = dalloc(h, ptr, n);
    if (rc) {
        ptr = nullptr;
        (void)hipGetLastError();
    }
    return rc;
}

// contacts, x0 and references of the current layout to the device.  x0_dev: x0's rows are on the
// device, x0_stride doubles apart (hsddp_update_problem_simulated).  meas: x0 is formed on the
// device from the measured records, behind the contacts' copy, and the handle keeps the records'
// foot placements (hsddp_update_problem_measured); every other x0 drops the ones it held.
static int upload_inputs(hsddp_handle h, const int *contacts, const double *x0, const double *ref_x,
                         const double *ref_u, const double *ref_foot, bool x0_dev = false, size_t x0_stride = NX,
                         const Measured *meas = nullptr)
{
    if (!h || (!x0 && !meas)) return fail(HSDDP_ERR_ARG, "null argument");
    const bool keep_refs = !ref_x && !ref_u && !ref_foot;
    if (!keep_refs && (!ref_x || !ref_u || !ref_foot)) return fail(HSDDP_ERR_ARG, "references: all three or none");
    if (keep_refs && !h->refs_on_device)
        return fail(HSDDP_ERR_ARG, "no device references for this layout (hsddp_build_references)");
    if (!h->lays.empty() && h->Bref == 1 && h->p.B > 1)  // a shared reference is laid out for one layout
        return fail(HSDDP_ERR_ARG, "per-element layouts need per-element references (desc.ref_per_element = 1)");
    HIPCHK(hipSetDevice(h->desc.device));
    const Params &p = h->p;
    const size_t B = p.B, S = p.S, P = p.P, Br = h->Bref;
    // contacts NULL: the handle's own (those hsddp_advance derived for this layout)
    const std::vector<int> own = contacts ? std::vector<int>() : h->contacts;
    if (!contacts) {
        if (!h->contacts_current || own.size() != B * (P + 1) * 4)
            return fail(HSDDP_ERR_ARG, "no contacts of this layout on the handle");
        contacts = own.data();
    }
    for (size_t q = 0; q < B * (P + 1) * 4; ++q)
        if (contacts[q] != 0 && contacts[q] != 1) return fail(HSDDP_ERR_ARG, "contacts must be 0/1");
    int rc;
    if (meas && ((!meas->on_device && (rc = measured_alloc(h, h->meas_states, B))) ||
                 (rc = measured_alloc(h, h->meas_feet, B * 12))))
        return rc;
    if ((rc = h2d((void *)h->d.contacts, contacts, B * (P + 1) * 4 * sizeof(int), h->stream))) return rc;
    if (meas) {
        const hsddp_robot_state *ds = meas->states;
        if (!meas->on_device) {
            if ((rc = h2d(h->meas_states, meas->states, B * sizeof(hsddp_robot_state), h->stream))) return rc;
            ds = h->meas_states;
        }
        launch_hkd_state(ds, h->d.contacts, (int)(P + 1) * 4, (double *)h->d.x0, (int)B, h->stream);
        HIPCHK(hipGetLastError());
        // the feet: 48 of every 144 bytes
        h->meas_held = false;
        HIPCHK(hipMemcpy2DAsync(h->meas_feet, 12 * sizeof(float), (const char *)ds + offsetof(hsddp_robot_state, foot_placements),
                                sizeof(hsddp_robot_state), 12 * sizeof(float), B, hipMemcpyDeviceToDevice, h->stream));
    } else if (x0_dev)
        HIPCHK(hipMemcpy2DAsync((void *)h->d.x0, NX * sizeof(double), x0, x0_stride * sizeof(double), NX * sizeof(double), B,
                                hipMemcpyDeviceToDevice, h->stream));
    else if ((rc = h2d((void *)h->d.x0, x0, B * NX * sizeof(double), h->stream)))
        return rc;
    h->meas_held = meas != nullptr;
    if (!keep_refs &&
        ((rc = h2d((void *)h->d.ref_x, ref_x, Br * S * NX * sizeof(double), h->stream)) ||
         (rc = h2d((void *)h->d.ref_u, ref_u, Br * S * NX * sizeof(double), h->stream)) ||
         (rc = h2d((void *)h->d.ref_foot, ref_foot, Br * S * 12 * sizeof(double), h->stream))))
        return rc;
    if (!keep_refs) {
        h->refs_on_device = false;
        h->ref_cols_stale = true;
    }
    h->contacts.assign(contacts, contacts + B * (P + 1) * 4);
    h->contacts_current = true;
    return HSDDP_OK;
}

extern "C" int hsddp_upload_problem(hsddp_handle h, const int *contacts, const double *x0, const double *ref_x,
                                    const double *ref_u, const double *ref_foot)
{
    int rc = upload_inputs(h, contacts, x0, ref_x, ref_u, ref_foot);
    if (rc) return rc;
    const Params &p = h->p;
    const size_t B = p.B, S = p.S, Br = h->Bref;
    // default warm start: Xbar = X = reference (HKDProblem.cpp:84-90), Ubar = U = 0, K = 0
    HIPCHK(hipMemsetAsync(h->d.sel, 0, B * sizeof(int), h->stream));  // nominal and working rows in buffer 0
    if (Br == 1) launch_broadcast(h->d.X3, h->d.ref_x, S * NX, B, h->stream);
    else HIPCHK(hipMemcpyAsync(h->d.X3, h->d.ref_x, B * S * NX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d.U3, 0, B * p.Kc * NX * sizeof(double), h->stream));
    if (p.fp32) HIPCHK(hipMemsetAsync(h->d.K32, 0, B * p.Kc * KCW * sizeof(float), h->stream));
    else HIPCHK(hipMemsetAsync(h->d.K, 0, B * p.Kc * KCW * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_problem = true;
    h->need_inputs = false;
    return hsddp_upload_warm_start(h, nullptr, nullptr, nullptr);  // (a new policy: the simulation held is stale)
}

// params (a new problem: hsddp_upload_warm_start): the working trajectory restarts at the warm
// start (X = Xbar, U = Ubar, Defect = 0), the ReB / AL parameters and touchdown constraints return
// to their initial values and the constraint values to zero — else all of them are kept.  A new
// problem zeroes dX, du and dU; an update keeps them, except that dX is zeroed under single
// shooting (the reasons stand at the memsets below).  Either way the per-element solver state is
// cleared and pending touchdown masks are resolved from the contact rows.
static int reset_working(hsddp_handle h, bool params)
{
    const Params &p = h->p;
    const size_t B = p.B, S = p.S, Kc = p.Kc;
    Bufs &d = h->d;
    if (params) launch_reset_working(p, d, h->stream);  // X = Xbar, U = Ubar (one buffer), Defect = 0
    // dX, du, dU: a new problem's are zero.  Between solves the initial rollout (eps = 0) does not
    // read them (fma_step / add_step) and the sweep and linear rollout rewrite them before any
    // trial, so an update keeps them (474 MB of memsets at B = 4096 saved per MPC tick; the shift
    // moves their rows with the knots, DESIGN.md "MPC tick") — except dX
    // with single shooting, which no linear rollout writes: the trials read it (zero, as in a
    // problem that never ran multiple shooting; the reference's is never written there either)
    if (params || p.ms0) HIPCHK(hipMemsetAsync(d.dX, 0, B * S * NX * sizeof(double), h->stream));
    if (params) {
        HIPCHK(hipMemsetAsync(d.du, 0, B * Kc * NX * sizeof(double), h->stream));
        HIPCHK(hipMemsetAsync(d.dU, 0, B * Kc * NX * sizeof(double), h->stream));
    }
    if (params) {
        launch_init_params(p, d, h->stream);
        h->reb_at_init = true;
        fill_params(h);
    }
    launch_resolve_td(p, d, h->stream);
    launch_reset_elements(p, d, h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->slots_fresh = false;
    return HSDDP_OK;
}

extern "C" int hsddp_update_problem(hsddp_handle h, const int *contacts, const double *x0, const double *ref_x,
                                    const double *ref_u, const double *ref_foot)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    int rc = upload_inputs(h, contacts, x0, ref_x, ref_u, ref_foot);
    if (rc) return rc;
    h->need_inputs = false;
    // keeps Xbar / Ubar / K, the working trajectory (X, U, Defect) and the constraint objects —
    // their ReB / AL parameters (HKDProblem::update's reset_params is a no-op, ConstraintsBase.h:
    // 165-167,341-348) and stored values — as the reference's objects live on into the next tick;
    // resets the per-element solver state; touchdown constraints added by the shift take their legs
    // from the new contact rows
    return reset_working(h, false);
}

static_assert(sizeof(hsddp_robot_state) == 144 && offsetof(hsddp_robot_state, foot_placements) == 96,
              "hsddp_robot_state is 144 bytes, the feet its last 48 (include/hsddp.h)");

// records [n] readable on `device`: what the HIP runtime knows of the pointer
static int check_device_records(const void *ptr, size_t n, int device)
{
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HSDDP_ERR_ARG, "states: not a device pointer");
    }
    if ((at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) || at.device != device)
        return fail(HSDDP_ERR_ARG, "states: not device memory of the handle's device");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HSDDP_ERR_ARG, "states: not a device allocation");
    }
    const size_t off = (size_t)((const char *)ptr - (const char *)base);
    if (off > size || n * sizeof(hsddp_robot_state) > size - off)
        return fail(HSDDP_ERR_ARG, "states: the device allocation holds fewer than B records");
    return HSDDP_OK;
}

extern "C" int hsddp_update_problem_measured(hsddp_handle h, const int *contacts, const hsddp_robot_state *states,
                                             int states_on_device, const double *ref_x, const double *ref_u,
                                             const double *ref_foot)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (!states) return fail(HSDDP_ERR_ARG, "null argument");
    if (states_on_device != 0 && states_on_device != 1) return fail(HSDDP_ERR_ARG, "states_on_device must be 0 or 1");
    if (states_on_device) {
        HIPCHK(hipSetDevice(h->desc.device));
        if (int rc = check_device_records(states, (size_t)h->p.B, h->desc.device)) return rc;
    }
    const Measured meas{states, states_on_device};
    int rc = upload_inputs(h, contacts, nullptr, ref_x, ref_u, ref_foot, false, NX, &meas);
    if (rc) return rc;
    h->need_inputs = false;
    return reset_working(h, false);  // (as hsddp_update_problem; its synchronisation ends the reads of `states`)
}

// ---- policy simulation -----------------------------------------------------------------------
static_assert(sizeof(hsddp_sim_sample) == 32, "hsddp_sim_sample is 32 bytes (include/hsddp.h)");

extern "C" int hsddp_simulate_policy(hsddp_handle h, int n_samples, int n_steps, const double *x_init, double *x_end,
                                     hsddp_sim_sample *summary, double *X, double *U)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (h->need_inputs) return fail(HSDDP_ERR_ARG, "the layout changed (hsddp_shift): call hsddp_update_problem first");
    if (n_samples < 1) return fail(HSDDP_ERR_ARG, "n_samples must be >= 1");
    if (n_steps < 1 || n_steps > h->p.Kc) return fail(HSDDP_ERR_ARG, "n_steps must lie in 1 .. Kc");
    if ((X != nullptr) != (U != nullptr)) return fail(HSDDP_ERR_ARG, "X and U: both or neither");
    const Params &p = h->p;
    const size_t rows = (size_t)p.B * n_samples;
    if ((size_t)p.B * (((size_t)n_samples + 63) / 64) > 0x7fffffffu) return fail(HSDDP_ERR_ARG, "too many samples");
    HIPCHK(hipSetDevice(h->desc.device));
    // x_end | x_init | summary | X | U, each piece a multiple of 32 bytes
    const size_t nx = rows * NX * sizeof(double), ns = rows * sizeof(hsddp_sim_sample),
                 nt = X ? rows * n_steps * NX * sizeof(double) : 0;
    const size_t need = 2 * nx + ns + 2 * nt;
    if (need > h->sim_bytes) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->sim_buf) hipFree(h->sim_buf);
        h->bytes -= h->sim_bytes;
        h->sim_buf = nullptr;
        h->sim_bytes = 0;
        h->sim_M = h->sim_n = 0;  // (the end states held went with the buffer)
        const hipError_t e = hipMalloc((void **)&h->sim_buf, need);
        if (e != hipSuccess) {
            h->sim_buf = nullptr;
            (void)hipGetLastError();
            return fail(HSDDP_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        h->sim_bytes = need;
        h->bytes += need;
    }
    SimArgs a{};
    a.M = n_samples;
    a.n_steps = n_steps;
    a.x_end = (double *)h->sim_buf;
    double *xi = (double *)(h->sim_buf + nx);
    a.summary = (hsddp_sim_sample *)(h->sim_buf + 2 * nx);
    if (X) {
        a.X = (double *)(h->sim_buf + 2 * nx + ns);
        a.U = (double *)(h->sim_buf + 2 * nx + ns + nt);
        HIPCHK(hipMemsetAsync(a.X, 0, 2 * nt, h->stream));  // rows past a diverged sample's break knot stay zero
    }
    h->sim_M = h->sim_n = 0;  // the held end states are being overwritten
    int rc;
    if (x_init) {
        if ((rc = h2d(xi, x_init, nx, h->stream))) return rc;
        a.x_init = xi;
    }
    // HSDDP_SIMULATE_TIMING=1: the kernel's device time (HIP events) to stderr (a diagnostic)
    static const bool timing = std::getenv("HSDDP_SIMULATE_TIMING") != nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timing) {
        HIPCHK(hipEventCreate(&ev[0]));
        HIPCHK(hipEventCreate(&ev[1]));
        HIPCHK(hipEventRecord(ev[0], h->stream));
    }
    if ((rc = sync_terrain(h)) || (rc = sync_weights(h)) || (rc = sync_phase_weights(h))) return rc;
    launch_simulate_policy(p, h->d, a, terrain_of(h), weights_of(h), h->stream);
    HIPCHK(hipGetLastError());
    if (timing) {
        float ms = 0;
        HIPCHK(hipEventRecord(ev[1], h->stream));
        HIPCHK(hipEventSynchronize(ev[1]));
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        hipEventDestroy(ev[0]);
        hipEventDestroy(ev[1]);
        std::fprintf(stderr, "hsddp_simulate_policy kernel ms: %.4f (B %d, M %d, n %d)\n", ms, p.B, n_samples, n_steps);
    }
    if (x_end) HIPCHK(hipMemcpyAsync(x_end, a.x_end, nx, hipMemcpyDeviceToHost, h->stream));
    if (summary) HIPCHK(hipMemcpyAsync(summary, a.summary, ns, hipMemcpyDeviceToHost, h->stream));
    if (X) {
        HIPCHK(hipMemcpyAsync(X, a.X, nt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(U, a.U, nt, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->sim_M = n_samples;
    h->sim_n = n_steps;
    h->sim_shifted = 0;
    h->sim_fresh = true;
    return HSDDP_OK;
}

extern "C" int hsddp_update_problem_simulated(hsddp_handle h, int sample)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (!h->sim_buf || h->sim_M < 1) return fail(HSDDP_ERR_ARG, "no simulation held (hsddp_simulate_policy)");
    if (!h->sim_fresh) return fail(HSDDP_ERR_ARG, "the simulation held is stale (a solve or warm-start upload since)");
    if (sample < 0 || sample >= h->sim_M) return fail(HSDDP_ERR_ARG, "sample outside 0 .. n_samples - 1");
    if (h->sim_shifted != h->sim_n)
        return fail(HSDDP_ERR_ARG, "the steps advanced since the simulation differ from its n_steps");
    const double *x0 = (const double *)h->sim_buf + (size_t)sample * NX;
    int rc = upload_inputs(h, nullptr, x0, nullptr, nullptr, nullptr, true, (size_t)h->sim_M * NX);
    if (rc) return rc;
    h->need_inputs = false;
    return reset_working(h, false);
}

extern "C" int hsddp_upload_warm_start(hsddp_handle h, const double *Xbar, const double *Ubar, const double *K)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    h->slots_fresh = false;
    h->sim_fresh = false;
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    HIPCHK(hipSetDevice(h->desc.device));
    const Params &p = h->p;
    const size_t B = p.B, S = p.S, Kc = p.Kc;
    Bufs &d = h->d;
    int rc;
    launch_normalize(p, d, h->stream);  // every element's nominal rows in buffer 0
    if (Xbar && (rc = h2d(d.X3, Xbar, B * S * NX * sizeof(double), h->stream))) return rc;
    if (Ubar && (rc = h2d(d.U3, Ubar, B * Kc * NX * sizeof(double), h->stream))) return rc;
    if (K) { // keep the 12 coupled rows of each knot's gain (KCW layout, hsddp_internal.h)
        std::vector<double> kc(B * Kc * KCW);
        for (size_t b = 0; b < B; ++b)
            for (size_t k = 0; k < Kc; ++k)
                for (int q = 0; q < 12; ++q) {
                    const int u = coupled_control(h, b, k, q);
                    std::memcpy(&kc[((b * Kc + k) * 12 + q) * NX], K + ((b * Kc + k) * NX + u) * NX, NX * sizeof(double));
                }
        if (p.fp32) {
            std::vector<float> k32(kc.begin(), kc.end());
            if ((rc = h2d(d.K32, k32.data(), B * Kc * KCW * sizeof(float), h->stream))) return rc;
            HIPCHK(hipStreamSynchronize(h->stream));
        } else if ((rc = h2d(d.K, kc.data(), B * Kc * KCW * sizeof(double), h->stream))) {
            return rc;
        }
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return reset_working(h, true);
}

static_assert(MTD == HSDDP_MAX_TD, "touchdown constraint slots");

extern "C" int hsddp_upload_constraint_params(hsddp_handle h, const double *reb_delta, const double *reb_eps,
                                              const int *td_legs, const double *al_sigma, const double *al_lambda)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    const Params &p = h->p;
    const size_t nr = (size_t)p.B * p.Kc * 20, nt = (size_t)p.B * p.P * MTD;
    if (td_legs)
        for (size_t q = 0; q < nt; ++q)
            if (td_legs[q] < 0 || td_legs[q] > 15) return fail(HSDDP_ERR_ARG, "td_legs entries are 4-bit leg masks");
    HIPCHK(hipSetDevice(h->desc.device));
    const Bufs &d = h->d;
    int rc;
    if (td_legs) {  // merged on the device: TD_STALE and TD_PENDING are its own (k_upload_td)
        char *buf;
        if ((rc = scratch(h, nt * sizeof(int), &buf)) || (rc = h2d(buf, td_legs, nt * sizeof(int), h->stream))) return rc;
        launch_upload_td(p, d, (const int *)buf, h->stream);
        HIPCHK(hipGetLastError());
    }
    if ((reb_delta && (rc = h2d(d.reb_delta, reb_delta, nr * sizeof(double), h->stream))) ||
        (reb_eps && (rc = h2d(d.reb_eps, reb_eps, nr * sizeof(double), h->stream))) ||
        (al_sigma && (rc = h2d(d.al_sigma, al_sigma, nt * 4 * sizeof(double), h->stream))) ||
        (al_lambda && (rc = h2d(d.al_lambda, al_lambda, nt * 4 * sizeof(double), h->stream))))
        return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (reb_delta || reb_eps) {  // the uniform-ReB shortcut holds only while every knot has the initial pair
        bool at = true;
        for (size_t q = 0; q < nr && at; ++q)
            at = (!reb_delta || reb_delta[q] == p.grf_delta) && (!reb_eps || reb_eps[q] == p.grf_eps);
        h->reb_at_init = at && h->reb_at_init;
        if (at && reb_delta && reb_eps) h->reb_at_init = true;
        fill_params(h);
    }
    h->slots_fresh = false;  // the running / terminal costs change with the parameters
    return HSDDP_OK;
}

extern "C" int hsddp_download_constraint_params(hsddp_handle h, double *reb_delta, double *reb_eps, int *td_legs,
                                                double *al_sigma, double *al_lambda)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    const Params &p = h->p;
    const size_t nr = (size_t)p.B * p.Kc * 20, nt = (size_t)p.B * p.P * MTD;
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const Bufs &d = h->d;
    if (reb_delta) HIPCHK(hipMemcpy(reb_delta, d.reb_delta, nr * sizeof(double), hipMemcpyDeviceToHost));
    if (reb_eps) HIPCHK(hipMemcpy(reb_eps, d.reb_eps, nr * sizeof(double), hipMemcpyDeviceToHost));
    if (td_legs) {
        HIPCHK(hipMemcpy(td_legs, d.td_mask, nt * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < nt; ++q) td_legs[q] &= 15;  // (legs only: TD_STALE is the device's)
    }
    if (al_sigma) HIPCHK(hipMemcpy(al_sigma, d.al_sigma, nt * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (al_lambda) HIPCHK(hipMemcpy(al_lambda, d.al_lambda, nt * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

// The stored constraint values, formed on the host from what the device keeps (hsddp_internal.h):
// a knot's GRF values from its cf_u forces where cf_flag is set, else from its working control row;
// a touchdown constraint's residual is 0 while TD_STALE, else its phase end's (term_h, written by
// the last rollout or divergence fix-up from the working X_i[N]).
extern "C" int hsddp_download_constraint_values(hsddp_handle h, double *grf_g, double *td_h)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (grf_g && !h->contacts_current) return fail(HSDDP_ERR_ARG, "no contacts of this layout on the handle");
    const Params &p = h->p;
    const size_t B = p.B, Kc = p.Kc, P = p.P;
    int rc;
    std::vector<ElemState> el(B);
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(el.data(), h->d.el, B * sizeof(ElemState), hipMemcpyDeviceToHost));
    if (grf_g) {
        std::vector<double> U(B * Kc * NX), cfu(B * Kc * 12);
        std::vector<int> cff(B * Kc);
        if ((rc = hsddp_download_working(h, nullptr, U.data(), nullptr, nullptr, nullptr))) return rc;
        HIPCHK(hipMemcpy(cfu.data(), h->d.cf_u, cfu.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cff.data(), h->d.cf_flag, cff.size() * sizeof(int), hipMemcpyDeviceToHost));
        std::fill(grf_g, grf_g + B * Kc * 20, 0.0);
        for (size_t b = 0; b < B; ++b) {
            const Layout L = layout_of(h, b);
            for (int i = 0; i < L.P; ++i)
                for (int k = 0; k < L.N[i]; ++k) {
                    const size_t q = b * Kc + L.k0[i] + k;
                    const double *f = (el[b].ovr && cff[q]) ? &cfu[q * 12] : &U[q * NX];
                    const double mu = h->terrain.empty() ? p.mu : h->terrain[(b * P + i) * 2];
                    for (int l = 0; l < 4; ++l) {
                        if (!h->contacts[(b * (P + 1) + i) * 4 + l]) continue;
                        const double *fl = f + 3 * l;
                        double *g = grf_g + q * 20 + 5 * l;  // GRFConstraint rows (HKDConstraints.cpp:15-22)
                        g[0] = fl[2];
                        g[1] = -fl[0] + mu * fl[2];
                        g[2] = fl[0] + mu * fl[2];
                        g[3] = -fl[1] + mu * fl[2];
                        g[4] = fl[1] + mu * fl[2];
                    }
                }
        }
    }
    if (td_h) {
        std::vector<int> mask(B * P * MTD);
        std::vector<double> th(B * P * 4);
        HIPCHK(hipMemcpy(mask.data(), h->d.td_mask, mask.size() * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(th.data(), h->d.term_h, th.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b)
            for (size_t i = 0; i < P; ++i)
                for (int j = 0; j < MTD; ++j) {
                    const int m = mask[(b * P + i) * MTD + j];
                    for (int l = 0; l < 4; ++l)
                        td_h[((b * P + i) * MTD + j) * 4 + l] =
                            ((m >> l) & 1) && !(m & TD_STALE) ? th[(b * P + i) * 4 + l] : 0.0;
                }
    }
    return HSDDP_OK;
}

// ---- per-phase terrain ---------------------------------------------------------------------------
// The host rows are the source of truth (hsddp_handle.h); the kernels' copy follows by sync_terrain.
extern "C" int hsddp_set_terrain(hsddp_handle h, const double *mu, const double *ground)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    const size_t B = h->p.B, P = h->p.P;
    const double fill[2] = {h->desc.cparams.mu_fric, h->desc.cparams.ground_height};
    std::vector<double> rows;
    if (mu || ground) {
        rows.resize(B * P * 2);
        for (size_t b = 0; b < B; ++b) {
            const size_t Pb = layout_of(h, b).P;
            for (size_t i = 0; i < P; ++i) {
                const bool own = i < Pb;  // (rows past the element's phases are not read)
                const double m = own && mu ? mu[b * P + i] : fill[0], g = own && ground ? ground[b * P + i] : fill[1];
                if (!std::isfinite(m) || !std::isfinite(g)) return fail(HSDDP_ERR_ARG, "terrain: a value is not finite");
                if (own && mu && !(m > 0)) return fail(HSDDP_ERR_ARG, "terrain: a friction coefficient is not positive");
                rows[(b * P + i) * 2] = m;
                rows[(b * P + i) * 2 + 1] = g;
            }
        }
    }
    if (!rows.empty())
        if (int rc = ensure_terrain_table(h)) return rc;
    // (the iteration graphs are keyed on the table pointer: off and on find their own)
    h->terrain.swap(rows);
    h->terrain_stale = true;
    h->slots_fresh = false;  // the stored slot costs were formed with the old friction coefficients
    return HSDDP_OK;
}

extern "C" int hsddp_get_terrain(hsddp_handle h, double *mu, double *ground)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    const size_t n = (size_t)h->p.B * h->p.P;
    for (size_t q = 0; q < n; ++q) {
        if (mu) mu[q] = h->terrain.empty() ? h->desc.cparams.mu_fric : h->terrain[2 * q];
        if (ground) ground[q] = h->terrain.empty() ? h->desc.cparams.ground_height : h->terrain[2 * q + 1];
    }
    return HSDDP_OK;
}

int hsddp::ensure_terrain_table(hsddp_handle h)
{
    if (h->terrain_dev) return HSDDP_OK;
    const size_t cap = (size_t)h->p.B * HSDDP_MAX_PHASES * 2;
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipHostMalloc((void **)&h->terrain_pin, cap * sizeof(double), 0));
    HIPCHK(hipEventCreateWithFlags(&h->terrain_up, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->terrain_up, h->stream));
    return dalloc(h, h->terrain_dev, cap);
}

int hsddp::sync_terrain(hsddp_handle h)
{
    if (h->terrain.empty() || !h->terrain_stale) return HSDDP_OK;
    if (!h->terrain_dev) return fail(HSDDP_ERR_DEVICE, "terrain rows without a device table");
    const size_t bytes = h->terrain.size() * sizeof(double);
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipEventSynchronize(h->terrain_up));  // (the last upload has read the staging)
    std::memcpy(h->terrain_pin, h->terrain.data(), bytes);
    // HSDDP_TERRAIN_TIMING=1: the upload's device time (HIP events) to stderr (a diagnostic)
    static const bool timing = std::getenv("HSDDP_TERRAIN_TIMING") != nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timing) {
        HIPCHK(hipEventCreate(&ev[0]));
        HIPCHK(hipEventCreate(&ev[1]));
        HIPCHK(hipEventRecord(ev[0], h->stream));
    }
    HIPCHK(hipMemcpyAsync(h->terrain_dev, h->terrain_pin, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->terrain_up, h->stream));
    if (timing) {
        float ms = 0;
        HIPCHK(hipEventRecord(ev[1], h->stream));
        HIPCHK(hipEventSynchronize(ev[1]));
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        hipEventDestroy(ev[0]);
        hipEventDestroy(ev[1]);
        std::fprintf(stderr, "terrain upload ms: %.4f (%zu bytes)\n", ms, bytes);
    }
    h->terrain_stale = false;
    return HSDDP_OK;
}

// ---- per-robot weights -----------------------------------------------------------------------------
// The host rows are the source of truth (hsddp_handle.h); the kernels' copy follows by sync_weights.
void hsddp::weights_row(const hsddp_hkd_weights &w, Wts &r)
{
    for (int j = 0; j < 3; ++j) { r.qbase[j] = w.q_eul[j]; r.qbase[3 + j] = w.q_pos[j]; r.qbase[6 + j] = w.q_omega[j]; r.qbase[9 + j] = w.q_v[j]; }
    r.q_qJ = w.q_qJ;
    for (int j = 0; j < 24; ++j) r.qf_scale[j] = w.qf_scale[j];
    r.qf_gain = w.qf_gain; r.r_grf = w.r_grf; r.r_qJd = w.r_qJd;
    for (int j = 0; j < 3; ++j) r.foot_w[j] = w.foot_w[j];
    r.foot_gain = w.foot_gain; r.foot_term_cost = w.foot_term_cost; r.foot_term_grad = w.foot_term_grad;
    r.pad[0] = r.pad[1] = 0.0;
}

bool hsddp::weights_finite(const hsddp_hkd_weights &w)
{
    const double *f = (const double *)&w;
    for (int j = 0; j < NW; ++j)
        if (!std::isfinite(f[j])) return false;
    return true;
}

extern "C" int hsddp_set_element_weights(hsddp_handle h, const hsddp_hkd_weights *w, const int *mask)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    const size_t B = h->p.B;
    if (!w) {  // the table off: every robot back at the handle's weights
        if (h->weights.empty()) return HSDDP_OK;
        h->weights.clear();
        h->pw_stale = true;
        h->slots_fresh = false;
        return HSDDP_OK;
    }
    for (size_t b = 0; b < B; ++b)
        if ((!mask || mask[b]) && !weights_finite(w[b])) return fail(HSDDP_ERR_ARG, "element weights: a value is not finite");
    if (int rc = ensure_weights_table(h)) return rc;
    // (the iteration graphs are keyed on the table pointer: off and on find their own)
    bool changed = h->weights.empty();
    if (changed) h->weights.assign(B, h->desc.weights);  // robots never set read the handle's weights
    for (size_t b = 0; b < B; ++b) {
        if (mask && !mask[b]) continue;
        if (std::memcmp(&h->weights[b], &w[b], sizeof w[b])) changed = true;
        h->weights[b] = w[b];
    }
    if (changed) {
        h->weights_stale = true;
        h->pw_stale = true;      // (the phases without an override read the robot's row)
        h->slots_fresh = false;  // the stored slot costs were formed with the old weights
    }
    return HSDDP_OK;
}

extern "C" int hsddp_get_element_weights(hsddp_handle h, hsddp_hkd_weights *w)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (!w) return fail(HSDDP_ERR_ARG, "null output");
    for (size_t b = 0; b < (size_t)h->p.B; ++b) w[b] = weights_of(h, b);
    return HSDDP_OK;
}

int hsddp::ensure_weights_table(hsddp_handle h)
{
    if (h->weights_dev) return HSDDP_OK;
    HIPCHK(hipSetDevice(h->desc.device));
    // piece by piece: a call that failed half-way is taken up where it stopped, nothing allocated twice
    if (!h->weights_pin) HIPCHK(hipHostMalloc((void **)&h->weights_pin, (size_t)h->p.B * sizeof(Wts), 0));
    if (!h->weights_up) {
        HIPCHK(hipEventCreateWithFlags(&h->weights_up, hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->weights_up, h->stream));
    }
    return dalloc(h, h->weights_dev, (size_t)h->p.B);
}

int hsddp::sync_weights(hsddp_handle h)
{
    if (h->weights.empty() || !h->weights_stale) return HSDDP_OK;
    if (!h->weights_dev) return fail(HSDDP_ERR_DEVICE, "weight rows without a device table");
    const size_t B = h->p.B, bytes = B * sizeof(Wts);
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipEventSynchronize(h->weights_up));  // (the last upload has read the staging)
    for (size_t b = 0; b < B; ++b) weights_row(h->weights[b], h->weights_pin[b]);
    // HSDDP_WEIGHTS_TIMING=1: the upload's device time (HIP events) to stderr (a diagnostic)
    static const bool timing = std::getenv("HSDDP_WEIGHTS_TIMING") != nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timing) {
        HIPCHK(hipEventCreate(&ev[0]));
        HIPCHK(hipEventCreate(&ev[1]));
        HIPCHK(hipEventRecord(ev[0], h->stream));
    }
    HIPCHK(hipMemcpyAsync(h->weights_dev, h->weights_pin, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->weights_up, h->stream));
    if (timing) {
        float ms = 0;
        HIPCHK(hipEventRecord(ev[1], h->stream));
        HIPCHK(hipEventSynchronize(ev[1]));
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        hipEventDestroy(ev[0]);
        hipEventDestroy(ev[1]);
        std::fprintf(stderr, "weights upload ms: %.4f (%zu bytes)\n", ms, bytes);
    }
    h->weights_stale = false;
    return HSDDP_OK;
}

// ---- per-phase weights -----------------------------------------------------------------------------
// The host flags and rows are the source of truth (hsddp_handle.h); the kernels' dense table of
// effective rows follows by sync_phase_weights.
extern "C" int hsddp_set_phase_weights(hsddp_handle h, const hsddp_hkd_weights *w, const int *mask)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    const size_t B = h->p.B, P = h->p.P;
    if (!w) {  // every override gone: the handle as one that never called this
        drop_phase_weights(h);
        return HSDDP_OK;
    }
    bool any = false;
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < (size_t)layout_of(h, b).P; ++i) {
            if (mask && !mask[b * P + i]) continue;
            any = true;
            if (!weights_finite(w[b * P + i])) return fail(HSDDP_ERR_ARG, "phase weights: a value is not finite");
        }
    if (!any) return HSDDP_OK;
    if (int rc = ensure_phase_weights_table(h)) return rc;
    bool changed = false;
    if (h->pw_set.empty()) {
        h->pw_set.assign(B * P, 0);
        h->pw.assign(B * P * NW, 0.0);
    }
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < (size_t)layout_of(h, b).P; ++i) {
            const size_t q = b * P + i;
            if (mask && !mask[q]) continue;
            if (!h->pw_set[q] || std::memcmp(&h->pw[q * NW], &w[q], sizeof w[q])) changed = true;
            h->pw_set[q] = 1;
            std::memcpy(&h->pw[q * NW], &w[q], sizeof w[q]);
        }
    if (changed) {
        h->pw_stale = true;
        h->slots_fresh = false;  // the stored slot costs were formed with the old weights
    }
    return HSDDP_OK;
}

extern "C" int hsddp_get_phase_weights(hsddp_handle h, hsddp_hkd_weights *w, int *is_set)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (!w) return fail(HSDDP_ERR_ARG, "null output");
    const size_t B = h->p.B, P = h->p.P;
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < P; ++i) {
            w[b * P + i] = weights_of(h, b, (int)i);
            if (is_set) is_set[b * P + i] = h->pw_set.empty() ? 0 : h->pw_set[b * P + i];
        }
    return HSDDP_OK;
}

int hsddp::ensure_phase_weights_table(hsddp_handle h)
{
    if (h->pw_dev) return HSDDP_OK;
    HIPCHK(hipSetDevice(h->desc.device));
    // at the largest phase stride, so no layout change moves it; piece by piece, as ensure_weights_table
    const size_t cap = (size_t)h->p.B * HSDDP_MAX_PHASES;
    if (!h->pw_pin) HIPCHK(hipHostMalloc((void **)&h->pw_pin, cap * sizeof(PWts), 0));
    if (!h->pw_up) {
        HIPCHK(hipEventCreateWithFlags(&h->pw_up, hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->pw_up, h->stream));
    }
    return dalloc(h, h->pw_dev, cap);
}

void hsddp::adopt_phase_weights(hsddp_handle h, std::vector<int> &set, std::vector<double> &rows)
{
    h->pw_set.swap(set);
    h->pw.swap(rows);
    settle_phase_weights(h);
}

void hsddp::settle_phase_weights(hsddp_handle h)
{
    bool any = false;
    for (int f : h->pw_set) any = any || f;
    h->slots_fresh = false;
    if (!any) {  // the last override left: the handle as one without
        h->pw_set.clear();
        h->pw.clear();
        return;
    }
    h->pw_stale = true;
}

int hsddp::sync_phase_weights(hsddp_handle h)
{
    if (h->pw_set.empty() || !h->pw_stale) return HSDDP_OK;
    if (!h->pw_dev) return fail(HSDDP_ERR_DEVICE, "phase weight rows without a device table");
    const size_t B = h->p.B, P = h->p.P, bytes = B * P * sizeof(PWts);
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipEventSynchronize(h->pw_up));  // (the last upload has read the staging)
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < P; ++i) weights_row(weights_of(h, b, (int)i), h->pw_pin[b * P + i].row);
    // HSDDP_WEIGHTS_TIMING=1: the upload's device time (HIP events) to stderr (a diagnostic)
    static const bool timing = std::getenv("HSDDP_WEIGHTS_TIMING") != nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timing) {
        HIPCHK(hipEventCreate(&ev[0]));
        HIPCHK(hipEventCreate(&ev[1]));
        HIPCHK(hipEventRecord(ev[0], h->stream));
    }
    HIPCHK(hipMemcpyAsync(h->pw_dev, h->pw_pin, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->pw_up, h->stream));
    if (timing) {
        float ms = 0;
        HIPCHK(hipEventRecord(ev[1], h->stream));
        HIPCHK(hipEventSynchronize(ev[1]));
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        hipEventDestroy(ev[0]);
        hipEventDestroy(ev[1]);
        std::fprintf(stderr, "phase weights upload ms: %.4f (%zu bytes)\n", ms, bytes);
    }
    h->pw_stale = false;
    return HSDDP_OK;
}

extern "C" int hsddp_download_trajectory(hsddp_handle h, double *Xbar, double *Ubar, double *K)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t B = h->p.B, S = h->p.S, Kc = h->p.Kc;
    int rc;
    launch_normalize(h->p, h->d, h->stream);  // nominal rows in buffer 0
    HIPCHK(hipStreamSynchronize(h->stream));
    if ((rc = d2h(Xbar, h->d.X3, B * S * NX * 8)) || (rc = d2h(Ubar, h->d.U3, B * Kc * NX * 8)))
        return rc;
    if (K && h->need_inputs)
        return fail(HSDDP_ERR_ARG, "the layout changed (hsddp_shift): call hsddp_update_problem before downloading K");
    if (K) { // expand the coupled rows; the decoupled controls' rows are exactly zero
        std::vector<double> kc(B * Kc * KCW);
        if (h->p.fp32) {
            std::vector<float> k32(B * Kc * KCW);
            if ((rc = d2h(k32.data(), h->d.K32, B * Kc * KCW * 4))) return rc;
            std::copy(k32.begin(), k32.end(), kc.begin());
        } else if ((rc = d2h(kc.data(), h->d.K, B * Kc * KCW * 8))) {
            return rc;
        }
        std::memset(K, 0, B * Kc * NN * sizeof(double));
        for (size_t b = 0; b < B; ++b)
            for (size_t k = 0; k < Kc; ++k)
                for (int q = 0; q < 12; ++q) {
                    const int u = coupled_control(h, b, k, q);
                    std::memcpy(K + ((b * Kc + k) * NX + u) * NX, &kc[((b * Kc + k) * 12 + q) * NX], NX * sizeof(double));
                }
    }
    return HSDDP_OK;
}

// diagnostic builds (-DHSDDP_STAMPS=1): per-element in-kernel stamp sums [B][16]; not in hsddp.h
extern "C" int hsddp_debug_stamps(hsddp_handle h, unsigned long long *out)
{
    if (!h || !out) return fail(HSDDP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->d.dbg, h->p.B * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return HSDDP_OK;
}

extern "C" int hsddp_download_working(hsddp_handle h, double *X, double *U, double *Defect, double *dX, double *dU)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t B = h->p.B, S = h->p.S, Kc = h->p.Kc;
    int rc;
    if ((rc = d2h(dX, h->d.dX, B * S * NX * 8)) || (rc = d2h(dU, h->d.dU, B * Kc * NX * 8)))
        return rc;
    if (X || U || Defect) {  // each element's working rows from the buffer sel names
        std::vector<int> sel(B);
        HIPCHK(hipMemcpy(sel.data(), h->d.sel, B * sizeof(int), hipMemcpyDeviceToHost));
        for (int q = 0; q < 3; ++q) {
            std::vector<double> xb(X ? B * S * NX : 0), ub(U ? B * Kc * NX : 0), db(Defect ? B * S * NX : 0);
            if ((rc = d2h(X ? xb.data() : nullptr, h->d.X3 + q * h->d.xs3, B * S * NX * 8)) ||
                (rc = d2h(U ? ub.data() : nullptr, h->d.U3 + q * h->d.us3, B * Kc * NX * 8)) ||
                (rc = d2h(Defect ? db.data() : nullptr, h->d.D3 + q * h->d.xs3, B * S * NX * 8)))
                return rc;
            for (size_t b = 0; b < B; ++b) {
                if (((sel[b] >> 2) & 3) != q) continue;
                if (X) std::copy(xb.begin() + b * S * NX, xb.begin() + (b + 1) * S * NX, X + b * S * NX);
                if (U) std::copy(ub.begin() + b * Kc * NX, ub.begin() + (b + 1) * Kc * NX, U + b * Kc * NX);
                if (Defect) std::copy(db.begin() + b * S * NX, db.begin() + (b + 1) * S * NX, Defect + b * S * NX);
            }
        }
    }
    return HSDDP_OK;
}

extern "C" int hsddp_download_references(hsddp_handle h, double *ref_x, double *ref_u, double *ref_foot)
{
    if (!h || !ref_x || !ref_u || !ref_foot) return fail(HSDDP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t Br = h->Bref, S = h->p.S;
    int rc;
    if ((rc = d2h(ref_x, h->d.ref_x, Br * S * NX * 8)) || (rc = d2h(ref_u, h->d.ref_u, Br * S * NX * 8)) ||
        (rc = d2h(ref_foot, h->d.ref_foot, Br * S * 12 * 8)))
        return rc;
    return HSDDP_OK;
}

extern "C" int hsddp_download_element_info(hsddp_handle h, hsddp_element_info *info)
{
    if (!h || !info) return fail(HSDDP_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<ElemState> el(h->p.B);
    HIPCHK(hipMemcpy(el.data(), h->d.el, h->p.B * sizeof(ElemState), hipMemcpyDeviceToHost));
    for (int b = 0; b < h->p.B; ++b) {
        const ElemState &e = el[b];
        info[b].cost = e.cost; info[b].feas = e.feas; info[b].merit = e.merit;
        info[b].max_tconstr = e.max_t; info[b].max_pconstr = e.max_p;
        info[b].iters = e.iters; info[b].outer_iters = e.outer_iters; info[b].status = e.status;
        info[b].n_ls_trials = e.n_ls;
    }
    return HSDDP_OK;
}

extern "C" int hsddp_download_solver_info(hsddp_handle h, int capacity, float *cost, float *dyn_feas,
                                          float *eqn_feas, float *ineq_feas, int *count)
{
    if (!h || capacity < 0) return fail(HSDDP_ERR_ARG, "null handle or negative capacity");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const int B = h->p.B, hc = h->p.hcap;
    std::vector<ElemState> el(B);
    HIPCHK(hipMemcpy(el.data(), h->d.el, B * sizeof(ElemState), hipMemcpyDeviceToHost));
    std::vector<float> hv((size_t)B * hc * 4);
    HIPCHK(hipMemcpy(hv.data(), h->d.hist, hv.size() * sizeof(float), hipMemcpyDeviceToHost));
    float *outs[4] = {cost, dyn_feas, eqn_feas, ineq_feas};
    for (int b = 0; b < B; ++b) {
        const int n = std::min(el[b].hist_n, std::min(hc, capacity));
        if (count) count[b] = n;
        for (int f = 0; f < 4; ++f) {
            if (!outs[f]) continue;
            float *o = outs[f] + (size_t)b * capacity;
            for (int k = 0; k < capacity; ++k) o[k] = k < n ? hv[((size_t)b * hc + k) * 4 + f] : 0.0f;
        }
    }
    return HSDDP_OK;
}

// ---- the reference Trajectory's derived fields (TrajectoryManagement.h:49-81) ---------------
// The device keeps the LQ model of a knot in the compact record (hsddp_internal.h); these host
// routines expand it to the reference's dense blocks for callers that read them.


extern "C" int hsddp_download_lq(hsddp_handle h, double *A, double *Bm, double *l, double *lx, double *lu,
                                 double *lxx, double *luu)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const Params &p = h->p;
    const size_t B = p.B, Kc = p.Kc, S = p.S, W = p.fp32 ? LQW32 : LQW;
    std::vector<double> rec(B * Kc * W), cost(B * S);
    if (p.fp32) {
        std::vector<float> r32(B * Kc * W);
        HIPCHK(hipMemcpy(r32.data(), h->d.lq32, r32.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t q = 0; q < rec.size(); ++q) rec[q] = r32[q];
    } else {
        HIPCHK(hipMemcpy(rec.data(), h->d.lq, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (l) HIPCHK(hipMemcpy(cost.data(), h->d.slot_cost, cost.size() * sizeof(double), hipMemcpyDeviceToHost));
    const double dt = p.dt;
    for (size_t b = 0; b < B; ++b)
        for (size_t kc = 0; kc < Kc; ++kc) {
            const double *r = rec.data() + (b * Kc + kc) * W;
            const int i = phase_of_control(layout_of(h, b), (int)kc);
            const int *c = h->contacts.data() + (b * (p.P + 1) + i) * 4;
            const size_t o = (b * Kc + kc);
            if (A) {  // A = I + S (hkd_model.h: Se, Sw, dt at (3 + a, 9 + a))
                double *a = A + o * NN;
                std::fill(a, a + NN, 0.0);
                for (int j = 0; j < NX; ++j) a[j * NX + j] = 1.0;
                for (int rr = 0; rr < 3; ++rr)
                    for (int q = 0; q < 5; ++q) a[rr * NX + hkd::se_col(q)] += r[LQ_SE + 5 * rr + q];
                for (int q = 0; q < 3; ++q) a[(3 + q) * NX + 9 + q] += dt;
                for (int rr = 0; rr < 3; ++rr)
                    for (int q = 0; q < 17; ++q) a[(6 + rr) * NX + hkd::sw_col(q)] += r[sw_at(rr, q)];
            }
            if (Bm) {
                double *bb = Bm + o * NN;
                std::fill(bb, bb + NN, 0.0);
                for (int rr = 0; rr < 3; ++rr)
                    for (int q = 0; q < 12; ++q) bb[(6 + rr) * NX + q] = r[bw_at(rr, q)];
                for (int lg = 0; lg < 4; ++lg)
                    for (int a = 0; a < 3; ++a) {
                        bb[(9 + a) * NX + 3 * lg + a] = dt * c[lg] / hkd::kMass;
                        bb[(12 + 3 * lg + a) * NX + 12 + 3 * lg + a] = dt * (1.0 - c[lg]);
                    }
            }
            // the weights of the knot's phase in the kernels' form (its override, the robot's row, or the handle's)
            Wts wr;
            weights_row(weights_of(h, b, i), wr);
            if (l) l[o] = cost[b * S + kc + i];
            if (lx) for (int j = 0; j < NX; ++j) lx[o * NX + j] = r[LQ_LX + j];
            if (lu) for (int j = 0; j < NX; ++j) lu[o * NX + j] = r[LQ_LU + j];
            if (lxx) {  // dt Q + dt D^T Qfoot D (HKDCost.cpp:22-37; constant per phase)
                double *m = lxx + o * NN;
                std::fill(m, m + NN, 0.0);
                for (int j = 0; j < NX; ++j)
                    m[j * NX + j] = dt * (j < 12 ? wr.qbase[j] : wr.q_qJ * (1 - c[(j - 12) / 3]));
                for (int lg = 0; lg < 4; ++lg)
                    for (int a = 0; a < 3; ++a) {
                        const double w = c[lg] ? dt * (wr.foot_gain * wr.foot_w[a]) : 0.0;
                        const int pa = 3 + a, qa = 12 + 3 * lg + a;
                        m[pa * NX + pa] += w; m[qa * NX + qa] += w;
                        m[pa * NX + qa] -= w; m[qa * NX + pa] -= w;
                    }
            }
            if (luu) {  // dt R + dt ReB Hessian of the stance legs' GRF rows (SinglePhase.cpp:380-394)
                double *m = luu + o * NN;
                std::fill(m, m + NN, 0.0);
                for (int j = 0; j < NX; ++j) m[j * NX + j] = dt * (j < 12 ? wr.r_grf : wr.r_qJd);
                static const int ix[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
                for (int lg = 0; lg < 4; ++lg)
                    for (int a = 0; a < 3; ++a)
                        for (int e = 0; e < 3; ++e) m[(3 * lg + a) * NX + 3 * lg + e] += r[LQ_RB + 6 * lg + ix[a][e]];
            }
        }
    return HSDDP_OK;
}

extern "C" int hsddp_download_terminal(hsddp_handle h, double *Phi, double *Phix, double *Phixx, double *Px)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const Params &p = h->p;
    const size_t B = p.B, P = p.P;
    std::vector<double> term(B * P * TW), cost(B * p.S);
    HIPCHK(hipMemcpy(term.data(), h->d.term, term.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cost.data(), h->d.slot_cost, cost.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        const Layout L = layout_of(h, b);
        for (size_t i = 0; i < P; ++i) {
            const double *t = term.data() + (b * P + i) * TW;
            const size_t o = b * P + i;
            if ((int)i >= L.P) {  // past this element's phases
                if (Phi) Phi[o] = 0;
                if (Phix) std::fill(Phix + o * NX, Phix + (o + 1) * NX, 0.0);
                if (Phixx) std::fill(Phixx + o * NN, Phixx + (o + 1) * NN, 0.0);
                if (Px) std::fill(Px + o * NN, Px + (o + 1) * NN, 0.0);
                continue;
            }
            if (Phi) Phi[o] = cost[b * p.S + L.s0[i] + L.N[i]];
            if (Phix) std::copy(t + TM_PHIX, t + TM_PHIX + NX, Phix + o * NX);
            if (Phixx) std::copy(t + TM_PHIXX, t + TM_PHIXX + NN, Phixx + o * NN);
            if (Px) {
                if ((int)i + 1 < L.P) std::copy(t + TM_PX, t + TM_PX + NN, Px + o * NN);
                else std::fill(Px + o * NN, Px + (o + 1) * NN, 0.0);  // no reset after the last phase
            }
        }
    }
    return HSDDP_OK;
}

extern "C" int hsddp_set_value_export(hsddp_handle h, int on)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->desc.device));
    if (on && !h->value0) {
        const size_t n = (size_t)h->p.B * HSDDP_MAX_PHASES * (NX + NN);
        HIPCHK(hipMalloc(&h->value0, n * sizeof(double)));
        HIPCHK(hipMemset(h->value0, 0, n * sizeof(double)));
        HIPCHK(hipStreamSynchronize(nullptr));
        h->bytes += n * sizeof(double);
        h->d.value0 = h->value0;
    }
    h->p.store_value = on ? 1 : 0;
    fill_params(h);
    return HSDDP_OK;
}

extern "C" int hsddp_download_value(hsddp_handle h, double *G, double *H)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->value0 || !h->p.store_value) return fail(HSDDP_ERR_ARG, "value export is off (hsddp_set_value_export)");
    HIPCHK(hipSetDevice(h->desc.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t B = h->p.B, P = h->p.P;
    std::vector<double> v(B * P * (NX + NN));
    HIPCHK(hipMemcpy(v.data(), h->value0, v.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t o = 0; o < B * P; ++o) {
        // phases past the element's own layout (per-element layouts, or left from before a shift) are zero
        const bool live = (int)(o % P) < layout_of(h, o / P).P;
        const double *s = v.data() + o * (NX + NN);
        if (G) { if (live) std::copy(s, s + NX, G + o * NX); else std::fill(G + o * NX, G + (o + 1) * NX, 0.0); }
        if (H) { if (live) std::copy(s + NX, s + NX + NN, H + o * NN); else std::fill(H + o * NN, H + (o + 1) * NN, 0.0); }
    }
    return HSDDP_OK;
}

extern "C" int hsddp_synchronize(hsddp_handle h)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    return HSDDP_OK;
}

extern "C" size_t hsddp_device_bytes(hsddp_handle h) { return h ? h->bytes : 0; }

// ---- model primitives ------------------------------------------------------------------------
static int check_launch()
{
    HIPCHK(hipGetLastError());
    return HSDDP_OK;
}

extern "C" int hsddp_hkd_dynamics(const double *x, const double *u, const double *c, double dt, double *xn, int n,
                                  void *stream)
{
    if (!x || !u || !c || !xn || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_dynamics(x, u, c, dt, xn, n, (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_dynamics_partial(const double *x, const double *u, const double *c, double dt, double *A,
                                          double *B, int n, void *stream)
{
    if (!x || !u || !c || !A || !B || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_partial(x, u, c, dt, A, B, n, (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_foot_position(const double *x, const int *leg, double *p, int n, void *stream)
{
    if (!x || !leg || !p || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_foot(x, leg, p, nullptr, n, (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_state(const hsddp_robot_state *states, const int *contact, double *x, int n, void *stream)
{
    if (!states || !contact || !x || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_hkd_state(states, contact, 4, x, n, (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_foot_jacobian(const double *x, const int *leg, double *J, int n, void *stream)
{
    if (!x || !leg || !J || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_foot(x, leg, nullptr, J, n, (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_resetmap(const double *x, const int *c, const int *cn, double *xn, int n, void *stream)
{
    if (!x || !c || !cn || !xn || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_reset(x, c, cn, xn, nullptr, n, (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_resetmap_partial(const double *x, const int *c, const int *cn, double *Px, int n,
                                          void *stream)
{
    if (!x || !c || !cn || !Px || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_reset(x, c, cn, nullptr, Px, n, (hipStream_t)stream);
    return check_launch();
}

// weights / dt of a plugin primitive in the solver's parameter block (the kernels share the
// solver's cost helpers)
static Params plugin_params(const hsddp_hkd_weights &w, double dt)
{
    Params p{};
    p.dt = dt;
    for (int j = 0; j < 3; ++j) { p.qbase[j] = w.q_eul[j]; p.qbase[3 + j] = w.q_pos[j]; p.qbase[6 + j] = w.q_omega[j]; p.qbase[9 + j] = w.q_v[j]; }
    p.q_qJ = w.q_qJ;
    for (int j = 0; j < 24; ++j) p.qf_scale[j] = w.qf_scale[j];
    p.qf_gain = w.qf_gain; p.r_grf = w.r_grf; p.r_qJd = w.r_qJd;
    for (int j = 0; j < 3; ++j) p.foot_w[j] = w.foot_w[j];
    p.foot_gain = w.foot_gain; p.foot_term_cost = w.foot_term_cost; p.foot_term_grad = w.foot_term_grad;
    return p;
}
extern "C" int hsddp_hkd_running_cost(const double *x, const double *u, const int *c, const double *xr, const double *ur,
                                      const double *pf, const hsddp_hkd_weights *w, double dt, int terms, double *l,
                                      double *lx, double *lu, double *lxx, double *luu, int n, void *stream)
{
    if (!x || !u || !c || !xr || !ur || !pf || !w || n < 0 || (terms & ~3)) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_running_cost(plugin_params(*w, dt), x, u, c, xr, ur, pf, terms, l, lx, lu, lxx, luu, n,
                                     (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_terminal_cost(const double *x, const int *c, const double *xr, const double *pf,
                                       const hsddp_hkd_weights *w, int terms, double *Phi, double *Phix, double *Phixx,
                                       int n, void *stream)
{
    if (!x || !c || !xr || !pf || !w || n < 0 || (terms & ~3)) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_terminal_cost(plugin_params(*w, 0.0), x, c, xr, pf, terms, Phi, Phix, Phixx, n,
                                      (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_grf_constraint(const double *u, const int *c, double mu, double *g, double *gu, int n,
                                        void *stream)
{
    if (!u || !c || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_grf(u, c, mu, g, gu, n, (hipStream_t)stream);
    return check_launch();
}
extern "C" int hsddp_hkd_touchdown_constraint(const double *x, const int *c, const int *cn, double ground, double *h,
                                              double *hx, int n, void *stream)
{
    if (!x || !c || !cn || n < 0) return fail(HSDDP_ERR_ARG, "bad argument");
    if (n) launch_model_touchdown(x, c, cn, ground, h, hx, n, (hipStream_t)stream);
    return check_launch();
}

extern "C" void *hsddp_device_alloc(size_t bytes, int device)
{
    if (hipSetDevice(device) != hipSuccess) { g_err = "hipSetDevice failed"; return nullptr; }
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { g_err = "hipMalloc failed"; return nullptr; }
    return p;
}
extern "C" int hsddp_device_free(void *p)
{
    HIPCHK(hipFree(p));
    return HSDDP_OK;
}
extern "C" int hsddp_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return HSDDP_OK;
}
extern "C" int hsddp_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return HSDDP_OK;
}
extern "C" int hsddp_device_synchronize(int device)
{
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    return HSDDP_OK;
}
