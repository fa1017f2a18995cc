// hsddp_solve.cpp — the per-element-masked solve loop of the batched HS-DDP solver
// (MultiPhaseDDP::solve, MultiPhaseDDP.cpp:232-428): hsddp_solve and its split form
// hsddp_solve_begin / hsddp_iterate / hsddp_solve_end, the inner iteration's hipGraph cache and
// the stats.
#include <cstdlib>
#include <cstring>
#include <utility>

#include "hsddp_handle.h"

using namespace hsddp;

namespace {
struct Timer {
    hipStream_t st;
    bool on;
    std::vector<hipEvent_t> *pool;  // the handle's events, handed out in order (no create / destroy per launch)
    size_t used = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[5];  // lq, riccati, forward, other, linear
    // the last end() event, when nothing was launched since: the next begin() reuses it (an event
    // record costs the stream a ~5 us gap, and adjacent end / begin pairs were two)
    hipEvent_t pend = nullptr;
    hipEvent_t next()
    {
        if (used == pool->size()) {
            hipEvent_t e;
            hipEventCreate(&e);
            pool->push_back(e);
        }
        return (*pool)[used++];
    }
    void begin(int cat, hipEvent_t &e0)
    {
        if (!on) return;
        (void)cat;
        if (pend) {
            e0 = pend;
            pend = nullptr;
            return;
        }
        e0 = next();
        hipEventRecord(e0, st);
    }
    // launches outside the timed categories follow: the next begin() records its own event
    void cut() { pend = nullptr; }
    void end(int cat, hipEvent_t e0)
    {
        if (!on) return;
        hipEvent_t e1 = next();
        hipEventRecord(e1, st);
        ev[cat].push_back({e0, e1});
        pend = e1;
    }
    double total(int cat)
    {
        double t = 0;
        for (auto &pr : ev[cat]) {
            float ms = 0;
            hipEventElapsedTime(&ms, pr.first, pr.second);
            t += ms;
        }
        ev[cat].clear();
        return t;
    }
};
}  // namespace

static int count_active(hsddp_handle h, int which, int &n)
{
    HIPCHK(hipMemsetAsync(h->d.counter, 0, 4 * sizeof(int), h->stream));
    launch_count(h->p, h->d, which, h->stream);
    HIPCHK(hipMemcpyAsync(h->host_counter, h->d.counter, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    n = h->host_counter[which];
    return HSDDP_OK;
}

// The solve is split so a caller can time a fixed number of inner iterations:
//   hsddp_solve_begin  = initial hybrid_rollout(0) + update_nominal + compute_cost (MultiPhaseDDP.cpp:257-260)
//                        and the first outer-iteration prologue (:284-303)
//   hsddp_iterate      = n inner iterations (:304-381) for every still-active element
//   hsddp_solve_end    = outer epilogue: AL / ReB updates and tests (:383-408)
// hsddp_solve runs the complete reference loop with per-element early exits.
static int solve_check(hsddp_handle h)
{
    if (!h) return fail(HSDDP_ERR_ARG, "null handle");
    if (!h->have_problem) return fail(HSDDP_ERR_ARG, "upload the problem first");
    if (h->need_inputs) return fail(HSDDP_ERR_ARG, "the layout changed (hsddp_shift): call hsddp_update_problem first");
    HIPCHK(hipSetDevice(h->desc.device));
    h->sim_fresh = false;  // the policy changes: a simulation held is of the old one
    if (int rc = sync_terrain(h)) return rc;
    if (int rc = sync_weights(h)) return rc;
    return sync_phase_weights(h);
}

static std::vector<double> ls_steps(double alpha)
{
    // line-search step sizes exactly as `while (eps > 1e-3) { ...; eps *= alpha; }` evaluates them
    std::vector<double> trials;
    for (double eps = 1; eps > 1e-3; eps *= alpha) trials.push_back(eps);
    return trials;
}

// Bufs::ref_t refreshed from the reference rows if an upload changed them since (before any
// launch that reads the references; never inside a graph capture)
static void sync_ref_columns(hsddp_handle h)
{
    if (!h->ref_cols_stale) return;
    launch_ref_columns(h->p, h->d, h->Bref, h->stream);
    h->ref_cols_stale = false;
}

static void begin_launches(hsddp_handle h)
{
    if (h->p.trace) hipMemsetAsync(h->d.dbg, 0, (size_t)h->p.B * 16 * sizeof(unsigned long long), h->stream);
    sync_ref_columns(h);
    launch_reset_elements(h->p, h->d, h->stream);
    launch_rollout(h->p, h->d, 0.0, 0, 1, -1, budget_of(h), terrain_of(h), weights_of(h), h->stream);
    launch_decide(h->p, h->d, 0.0, 0, 1, -1, budget_of(h), terrain_of(h), weights_of(h), h->stream);
    h->slots_fresh = true;
}

static void iteration_launches(hsddp_handle h, const std::vector<double> &trials, Timer &tm)
{
    const Params &p = h->p;
    const Bufs &d = h->d;
    hipStream_t st = h->stream;
    hipEvent_t e0;
    tm.begin(0, e0);
    {   // every path to here ran a rollout on the working trajectory (the initial one or the last
        // line-search trial, quirk A2) unless the cost parameters changed since (slots_fresh)
        Params pl = p;
        pl.lq_slots = h->slots_fresh ? 0 : 1;
        launch_lq(pl, d, terrain_of(h), weights_of(h), st);
    }
    tm.end(0, e0);
    tm.begin(1, e0);
    launch_riccati(p, d, weights_of(h), st);
    tm.end(1, e0);
    // the linear rollout with multiple shooting only (MultiPhaseDDP.cpp:326-329); with single
    // shooting the sweep forms dV and the merit (k_riccati's DV instantiation)
    if (!p.ms0) {
        tm.begin(4, e0);
        launch_lin_rollout(p, d, weights_of(h), st);
        tm.end(4, e0);
    }
    tm.begin(2, e0);
    for (size_t t = 0; t < trials.size(); ++t) {
        launch_rollout(p, d, trials[t], t + 1 == trials.size(), 0, (int)t, budget_of(h), terrain_of(h), weights_of(h), st);
        launch_decide(p, d, trials[t], t + 1 == trials.size(), 0, (int)t, budget_of(h), terrain_of(h), weights_of(h), st);
    }
    tm.end(2, e0);
    h->slots_fresh = true;
}

// One early-exit inner iteration of hsddp_solve (MultiPhaseDDP.cpp:304-381 and the `n == 0` test)
// replayed from a hipGraph: the ~15 launches, the count kernel and the pinned read-back of the
// activity count go to the device as one submission.  At B = 1 (BASELINE config 1) the iteration's
// kernels are a few microseconds each and the host's per-launch cost was the critical path.  The
// graph freezes the launch arguments (Params, Bufs, the step sizes): it is re-captured whenever
// they differ from the ones it was built with.  The per-phase timers are not recorded in this mode
// (hsddp_stats carries ms_total only); HSDDP_NO_GRAPH=1 restores launch-by-launch issue.
static bool graphs_enabled()
{
    const char *e = std::getenv("HSDDP_NO_GRAPH");  // read per solve: a test switches it in-process
    return !(e && *e && *e != '0');
}

static int graph_launch(hsddp_handle h, const std::vector<double> &trials, int par)
{
    Params pl = h->p;
    pl.lq_slots = h->slots_fresh ? 0 : 1;
    hsddp_handle_t::IterGraph *hit = nullptr;
    for (auto &c : h->iter_graph)
        if (c.exec && c.par == par && !std::memcmp(&c.p, &pl, sizeof(Params)) &&
            !std::memcmp(&c.d, &h->d, sizeof(Bufs)) && c.alpha == h->opt.alpha && c.budget == budget_of(h) &&
            c.terrain == terrain_of(h) && c.weights == weights_of(h).robot && c.phase_weights == weights_of(h).phase)
            hit = &c;
    if (!hit) {
        auto &g = h->iter_graph[h->iter_graph_next];
        h->iter_graph_next = (h->iter_graph_next + 1) % 8;
        if (g.exec) {
            // the victim may be the iteration queued last (still on the stream): drain the stream
            // before its exec goes away (evictions are rare: 8 keys cover an MPC tick's recurring ones)
            HIPCHK(hipStreamSynchronize(h->stream));
            HIPCHK(hipGraphExecDestroy(g.exec));
        }
        g.exec = nullptr;
        HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        Timer off{h->stream, false, &h->events};
        iteration_launches(h, trials, off);
        launch_count(h->p, h->d, 1, h->stream);  // (k_lq's first terminal task zeroed the counts)
        hipError_t e = hipMemcpyAsync(h->host_counter + 8 + 4 * par, h->d.counter, 4 * sizeof(int), hipMemcpyDeviceToHost,
                               h->stream);
        hipGraph_t graph = nullptr;
        const hipError_t ec = hipStreamEndCapture(h->stream, &graph);
        if (e == hipSuccess) e = ec;
        if (e == hipSuccess) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        if (graph) hipGraphDestroy(graph);
        if (e != hipSuccess) {
            g.exec = nullptr;
            return fail(HSDDP_ERR_DEVICE, std::string("iteration graph: ") + hipGetErrorString(e));
        }
        std::memcpy(&g.p, &pl, sizeof(Params));
        std::memcpy(&g.d, &h->d, sizeof(Bufs));
        g.alpha = h->opt.alpha;
        g.budget = budget_of(h);
        g.terrain = terrain_of(h);  // (null: terrain off — other instantiations, other arguments)
        g.weights = weights_of(h).robot;  // (null: the table off)
        g.phase_weights = weights_of(h).phase;  // (null: no phase has an override)
        g.par = par;
        hit = &g;
    }
    if (!h->iter_done[par]) HIPCHK(hipEventCreateWithFlags(&h->iter_done[par], hipEventDisableTiming));
    HIPCHK(hipGraphLaunch(hit->exec, h->stream));
    HIPCHK(hipEventRecord(h->iter_done[par], h->stream));
    h->slots_fresh = true;
    return HSDDP_OK;
}

static int graph_wait(hsddp_handle h, int par, int &n_active)
{
    HIPCHK(hipEventSynchronize(h->iter_done[par]));
    n_active = h->host_counter[8 + 4 * par + 1];
    return HSDDP_OK;
}

static void outer_end_launches(hsddp_handle h, Timer &tm)
{
    hipEvent_t e0;
    tm.begin(3, e0);
    // update_REB_params moves per-knot (delta, eps) unless they stay uniform: the running costs change
    if (h->opt.ReB_active && !h->p.reb_uniform) {
        h->slots_fresh = false;
        h->reb_at_init = false;
    }
    if (h->opt.ReB_active) launch_reb_update(h->p, h->d, terrain_of(h), h->stream);
    launch_outer_end(h->p, h->d, budget_of(h), h->stream);
    tm.end(3, e0);
}

static int finish_stats(hsddp_handle h, Timer &tm, hipEvent_t e0, hsddp_stats *stats, int iters, int outers, int nbwd)
{
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!stats) return HSDDP_OK;
    hipEvent_t e1;
    hipEventCreate(&e1);
    hipEventRecord(e1, h->stream);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    stats->ms_total = ms;
    stats->ms_lq = tm.total(0);
    stats->ms_backward = tm.total(1);
    stats->ms_forward = tm.total(2);
    stats->ms_other = tm.total(3);
    stats->ms_linear = tm.total(4);
    stats->inner_iterations = iters;
    stats->outer_iterations = outers;
    stats->n_backward_launches = nbwd;
    // the two sums on the device (a copy of every element's state would be ~0.6 MB per call)
    HIPCHK(hipMemsetAsync(h->d.counter + 4, 0, 2 * sizeof(int), h->stream));
    launch_stat_sums(h->p, h->d, h->stream);
    HIPCHK(hipMemcpyAsync(h->host_counter + 4, h->d.counter + 4, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    stats->ls_trials = h->host_counter[4];
    stats->element_iterations = h->host_counter[5];
    return HSDDP_OK;
}

static hipEvent_t start_stats(hsddp_handle h, hsddp_stats *stats)
{
    if (!stats) return nullptr;
    memset(stats, 0, sizeof(*stats));
    hipEvent_t e0;
    hipEventCreate(&e0);
    hipEventRecord(e0, h->stream);
    return e0;
}

extern "C" int hsddp_solve(hsddp_handle h, hsddp_stats *stats)
{
    int rc = solve_check(h);
    if (rc) return rc;
    Timer tm{h->stream, stats != nullptr, &h->events};
    hipEvent_t e0 = start_stats(h, stats);
    const std::vector<double> trials = ls_steps(h->opt.alpha);
    begin_launches(h);
    int iters = 0, outers = 0, nbwd = 0;
    const bool checks = !h->opt.no_early_exit;
    const bool graph = checks && graphs_enabled();
    // the handle-wide bounds, or with per-element budgets the largest (an element past its own is inert)
    const int n_outer = outer_bound(h), n_inner = inner_bound(h);
    for (int ou = 0; ou < n_outer; ++ou) {
        tm.cut();
        launch_outer_begin(h->p, h->d, budget_of(h), h->stream);
        outers++;
        for (int in = 0; in < n_inner; ++in) {
            if (graph) {
                // iteration `in` was launched by the step before (or here, for the first); the next
                // one is queued before waiting for this one's count, so the GPU never waits on the
                // host's round trip.  When the count comes back 0 the queued iteration finds every
                // element inner_done / done and returns at once (the kernels' own early exits), as
                // the reference's loop would not have run it; it is never queued past max_DDP_iter.
                int n = 0;
                tm.cut();
                if (in == 0 && (rc = graph_launch(h, trials, 0))) return rc;
                if (in + 1 < n_inner && (rc = graph_launch(h, trials, (in + 1) & 1))) return rc;
                if ((rc = graph_wait(h, in & 1, n))) return rc;
                iters++;
                nbwd++;
                if (n == 0) break;
                continue;
            }
            iteration_launches(h, trials, tm);
            iters++;
            nbwd++;
            if (checks) {
                int n = 0;
                tm.cut();
                if ((rc = count_active(h, 1, n))) return rc;
                if (n == 0) break;
            }
        }
        outer_end_launches(h, tm);
        if (checks) {
            int n = 0;
            tm.cut();
            if ((rc = count_active(h, 2, n))) return rc;
            if (n == 0) break;
        }
    }
    return finish_stats(h, tm, e0, stats, iters, outers, nbwd);
}

extern "C" int hsddp_solve_begin(hsddp_handle h)
{
    int rc = solve_check(h);
    if (rc) return rc;
    begin_launches(h);
    launch_outer_begin(h->p, h->d, budget_of(h), h->stream);
    HIPCHK(hipGetLastError());
    return HSDDP_OK;
}

extern "C" int hsddp_iterate(hsddp_handle h, int n, hsddp_stats *stats)
{
    int rc = solve_check(h);
    if (rc) return rc;
    if (n < 0) return fail(HSDDP_ERR_ARG, "negative iteration count");
    Timer tm{h->stream, stats != nullptr, &h->events};
    hipEvent_t e0 = start_stats(h, stats);
    const std::vector<double> trials = ls_steps(h->opt.alpha);
    sync_ref_columns(h);  // (references uploaded after hsddp_solve_begin)
    for (int i = 0; i < n; ++i) iteration_launches(h, trials, tm);
    return finish_stats(h, tm, e0, stats, n, 0, n);
}

extern "C" int hsddp_solve_end(hsddp_handle h)
{
    int rc = solve_check(h);
    if (rc) return rc;
    Timer tm{h->stream, false, &h->events};
    outer_end_launches(h, tm);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return HSDDP_OK;
}
