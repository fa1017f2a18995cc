// hsddp_phases.cpp — phase layouts and HKDProblem::update's bookkeeping on the host (hsddp_phases.h).
#include "hsddp_phases.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>

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

// ---- elements grouped by an integer key ---------------------------------------------------------
std::vector<int> layout_key(const Layout &L, bool with_ss)
{
    std::vector<int> key(L.N, L.N + L.P);
    if (with_ss) {
        key.push_back(-1);
        key.insert(key.end(), L.ss, L.ss + L.P);
    }
    return key;
}

std::vector<int> shift_key(const Layout &L, const int *reach, int n_steps, const int *cc)
{
    std::vector<int> key = layout_key(L, true);
    key.insert(key.end(), reach, reach + L.P);
    key.insert(key.end(), cc, cc + n_steps);
    return key;
}

// ---- the shift ----------------------------------------------------------------------------------
int plan_shift(const HorizonView &v, int n_steps, const int *cc, size_t bstride, ShiftPlan &plan, std::string &why)
{
    const size_t B = v.B;
    Interner keys;
    plan.map_id.assign(B, 0);
    // the shared layout shifted by one set of flags (hsddp_shift): one key for the batch
    // (a per-element key and map lookup cost ≈ 1 µs an element: 4 ms of host time at B = 4096)
    const size_t nkey = (!v.lays && bstride == 0) ? std::min<size_t>(B, 1) : B;
    for (size_t b = 0; b < nkey; ++b) {
        const Layout &L = v.layout(b);
        const int *flags = cc + b * bstride;
        const int seen = keys.size();
        plan.map_id[b] = keys(shift_key(L, v.reach_of(b), n_steps, flags));
        if (plan.map_id[b] < seen) continue;
        PhaseStepper st(L, v.reach_of(b));
        Layout Ln;
        int rc = 0;
        for (int j = 0; j < n_steps && !rc; ++j)
            if (!(rc = st.drop_front("shift", why))) rc = st.extend_back(flags[j], "shift", why);
        if (rc || (rc = st.finish(Ln, why))) return rc;
        plan.phs.push_back(std::move(st.ph));
        plan.nl.push_back(Ln);
    }
    if (plan.phs.size() > 1 && v.Bref == 1 && B > 1) {
        why = "the elements' shifts diverge into per-element layouts, which need per-element "
              "references (ref_per_element = 1)";
        return HSDDP_ERR_ARG;
    }
    return HSDDP_OK;
}

int flatten_shift(const ShiftPlan &plan, int Kc, size_t S_cap, ShiftMaps &m, std::string &why)
{
    const int nk = (int)plan.phs.size();
    m.S_new = m.P_new = 0;
    for (const Layout &L : plan.nl) {
        if (control_slots(L) != Kc || (size_t)L.S > S_cap) {
            why = "shifted layout exceeds the handle's capacity";
            return HSDDP_ERR_ARG;
        }
        m.S_new = std::max(m.S_new, L.S);
        m.P_new = std::max(m.P_new, L.P);
    }
    m.smap.assign((size_t)nk * m.S_new, -1);
    m.cmap.assign((size_t)nk * Kc, 0);
    m.rmap.assign((size_t)nk * Kc, 0);
    m.pmap.assign((size_t)nk * MAXP, -1);
    m.nadd.assign((size_t)nk * MAXP, 0);
    for (int q = 0; q < nk; ++q) {
        size_t s = 0, k = 0, r = 0;
        for (size_t i = 0; i < plan.phs[q].size(); ++i) {
            const ShiftPhase &f = plan.phs[q][i];
            for (int x : f.xs) m.smap[(size_t)q * m.S_new + s++] = x;
            for (int x : f.us) m.cmap[(size_t)q * Kc + k++] = x;
            for (int x : f.rs) m.rmap[(size_t)q * Kc + r++] = x;
            m.pmap[(size_t)q * MAXP + i] = f.src;
            m.nadd[(size_t)q * MAXP + i] = f.add;
        }
    }
    return HSDDP_OK;
}

void shifted_layouts(const ShiftPlan &plan, std::vector<Layout> &lays, std::vector<int> &reach)
{
    const size_t B = plan.map_id.size();
    lays.resize(B);
    reach.assign(B * MAXP, 0);
    for (size_t b = 0; b < B; ++b) {
        lays[b] = plan.nl[plan.map_id[b]];
        plan.reach(plan.map_id[b], &reach[b * MAXP]);
    }
}

// ---- terrain ---------------------------------------------------------------------------------------
void put_terrain_rows(const double *rows, int n, int P, const double *fill, double *out)
{
    for (int i = 0; i < P; ++i) {
        const double *src = rows && i < n ? rows + 2 * i : fill;
        out[2 * i] = src[0];
        out[2 * i + 1] = src[1];
    }
}

void shift_terrain(const HorizonView &v, const ShiftPlan &plan, int P, std::vector<double> &out)
{
    out.resize((size_t)v.B * P * 2);
    for (int b = 0; b < v.B; ++b) {
        const std::vector<ShiftPhase> &ph = plan.phs[plan.map_id[b]];
        double *row = &out[(size_t)b * P * 2];
        put_terrain_rows(nullptr, 0, P, v.fill, row);
        for (int i = 0; i < (int)ph.size() && i < P; ++i) {
            // (i = 0 without a source: an element whose rows the caller writes; they stay at fill)
            const double *src = ph[i].src >= 0 ? &v.terrain[((size_t)b * v.P + ph[i].src) * 2] : i > 0 ? row + 2 * (i - 1) : v.fill;
            row[2 * i] = src[0];
            row[2 * i + 1] = src[1];
        }
    }
}

// ---- per-phase weights ------------------------------------------------------------------------------
void put_phase_weight_rows(const int *set, const double *rows, int n, int P, int *out_set, double *out_rows)
{
    for (int i = 0; i < P; ++i) {
        const bool on = set && i < n && set[i];
        out_set[i] = on ? 1 : 0;
        if (on) std::copy_n(rows + (size_t)i * NW, NW, out_rows + (size_t)i * NW);
        else std::fill_n(out_rows + (size_t)i * NW, NW, 0.0);
    }
}

void shift_phase_weights(const HorizonView &v, const ShiftPlan &plan, int P, std::vector<int> &set, std::vector<double> &rows)
{
    set.assign((size_t)v.B * P, 0);
    rows.assign((size_t)v.B * P * NW, 0.0);
    for (int b = 0; b < v.B; ++b) {
        const std::vector<ShiftPhase> &ph = plan.phs[plan.map_id[b]];
        for (int i = 0; i < (int)ph.size() && i < P; ++i) {
            const int src = ph[i].src;
            if (src < 0 || src >= v.P || !v.pw_set[(size_t)b * v.P + src]) continue;
            set[(size_t)b * P + i] = 1;
            std::copy_n(&v.pw[((size_t)b * v.P + src) * NW], NW, &rows[((size_t)b * P + i) * NW]);
        }
    }
}

// ---- references ------------------------------------------------------------------------------------
std::vector<float> clock_starts(const Layout &L, float dt_sim)
{
    std::vector<float> start(L.P);
    float t = 0.0f;
    for (int i = 0; i < L.P; ++i) {
        start[i] = t;
        for (int k = 0; k < L.N[i]; ++k) t += dt_sim;
    }
    return start;
}

std::vector<int> slot_samples(const Layout &L, const std::vector<float> &start, float dt_sim, float dt_ref, int sz, int S)
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

int SlotMaps::add(const Layout &L, const float *phase_start_times, float dt_sim, float dt_ref, int sz, int S)
{
    const int seen = keys.size(), q = keys(layout_key(L, false));
    if (q < seen) return q;
    std::vector<float> start;
    if (phase_start_times)
        for (int i = 0; i < L.P; ++i) start.push_back(phase_start_times[i] - phase_start_times[0]);
    else
        start = clock_starts(L, dt_sim);
    const std::vector<int> row = slot_samples(L, start, dt_sim, dt_ref, sz, S);
    idx.insert(idx.end(), row.begin(), row.end());
    starts.push_back(std::move(start));
    return q;
}

void plan_refs(const HorizonView &v, const int *window_start, int window_len, const float *phase_start_times,
               float dt_sim, bool initial, RefPlan &out)
{
    const int sz = window_len - 1;
    SlotMaps maps;
    out.map_id.assign(v.lays ? v.B : 0, 0);
    for (int b = 0; b < (v.lays ? v.B : 1); ++b) {
        const int q = maps.add(v.layout(b), phase_start_times, dt_sim, v.ref_dt, sz, v.S);
        if (v.lays) out.map_id[b] = q;
    }
    out.idx.swap(maps.idx);
    if (!initial) return;
    out.durations.assign((size_t)v.B * v.P * 4, 0.0);
    for (int b = 0; b < v.B; ++b) {
        const std::vector<float> &start = maps.starts[v.lays ? out.map_id[b] : 0];
        for (int i = 0; i < (int)start.size(); ++i) {
            const int k = std::min(window_start[v.Bref == 1 ? 0 : b] + sample_at(start[i], v.ref_dt, sz), v.ref_n - 1);
            for (int l = 0; l < 4; ++l) out.durations[((size_t)b * v.P + i) * 4 + l] = v.table[k].status_dur[l];
        }
    }
}

// ---- hsddp_advance ---------------------------------------------------------------------------------
namespace {
// the table's sample at relative time t of element b's window, the windows starting at w
const hsddp_quad_state &window_sample(const HorizonView &v, const std::vector<int> &w, int b, float t)
{
    const int k = w[v.Bref == 1 ? 0 : b] + sample_at(t, v.ref_dt, v.win_len - 1);
    return v.table[std::min(k, v.ref_n - 1)];
}
float rel_at(const AdvanceWalk &w, int b, int j) { return w.relj[j][w.relj[j].size() == 1 ? 0 : b]; }
// a phase's sample: of an old phase its row of the view's contacts / durations, of one these steps
// start the table's at the horizon end of its first step
const int *phase_contact(const HorizonView &v, const AdvanceWalk &w, int b, const ShiftPhase &f)
{
    return f.src >= 0 ? &v.contacts[((size_t)b * (v.P + 1) + f.src) * 4]
                      : window_sample(v, w.wsj[f.born], b, rel_at(w, b, f.born)).contact;
}
const double *phase_duration(const HorizonView &v, const AdvanceWalk &w, int b, const ShiftPhase &f)
{
    return f.src >= 0 ? &v.durations[((size_t)b * v.P + f.src) * 4]
                      : window_sample(v, w.wsj[f.born], b, rel_at(w, b, f.born)).status_dur;
}
}  // namespace

int walk_advance(const HorizonView &v, int n_steps, float plan_duration, AdvanceWalk &w, std::string &why)
{
    const int B = v.B;
    const bool elem = v.lays != nullptr;
    int adv = 0;  // samples per simulation step
    for (int i = 1; approx_leq(i * v.ref_dt, v.dt_sim); ++i) adv++;
    // QuadReference::step for every step: the window starts and the clock (shared by the batch, or
    // each element's own once hsddp_restart_elements has set some element's back to 0)
    w.wsj.assign(n_steps, std::vector<int>());
    w.relj.assign(n_steps, std::vector<float>());
    w.ws.assign(v.win_start, v.win_start + v.Bref);
    w.t_cur = v.t_el ? std::vector<float>(v.t_el, v.t_el + B) : std::vector<float>(1, v.t_cur);
    for (int j = 0; j < n_steps; ++j) {
        for (int a = 0; a < adv; ++a) {
            for (float &t : w.t_cur) t += v.ref_dt;
            for (int &s : w.ws) s++;
        }
        for (int s : w.ws)
            if (s >= v.ref_n) { why = "the reference window ran past the table"; return HSDDP_ERR_ARG; }
        w.wsj[j] = w.ws;
        for (float t : w.t_cur) w.relj[j].push_back((t + plan_duration) - t);  // new_end_time - new_start_time
    }
    // the MPC batch of one gait: an element whose contact rows equal element 0's has its bookkeeping
    w.rep.resize(B);
    for (int b = 0; b < B; ++b) {
        const size_t n = (size_t)(v.P + 1) * 4;
        w.rep[b] = (b > 0 && !elem && v.Bref == 1 && std::equal(v.contacts + b * n, v.contacts + (b + 1) * n, v.contacts)) ? 0 : b;
    }
    // beside the phases: the step flags, where the next-contact row comes from and the slot map
    // (elements with equal layout, reach flags and step flags share one)
    w.el.assign(B, AdvanceWalk::Element());
    w.plan = ShiftPlan{};
    Interner keys;
    int rc;
    for (int b = 0; b < B; ++b) {
        if (w.rep[b] != b) continue;
        AdvanceWalk::Element &W = w.el[b];
        const Layout &L = v.layout(b);
        PhaseStepper st(L, v.reach_of(b));
        W.P_old = L.P;
        W.flags.assign(n_steps, 0);
        for (int j = 0; j < n_steps; ++j) {
            if ((rc = st.drop_front("advance", why))) return rc;
            const int *nc = window_sample(v, w.wsj[j], b, rel_at(w, b, j)).contact, *lc = phase_contact(v, w, b, st.ph.back());
            int cc = 0;
            for (int l = 0; l < 4; ++l) cc |= nc[l] != lc[l];
            if ((rc = st.extend_back(cc, "advance", why))) return rc;
            // a new phase carries no terminal constraint (identity reset)
            if (st.ph.back().born == j) { W.next_kind = 1; W.next_step = j; }
            if (st.ph.back().reach) { W.next_kind = 2; W.next_step = j; }
            W.flags[j] = cc;
        }
        if (b > 0 && !elem && W.flags == w.el[0].flags) continue;  // element 0's layout, reach flags and step flags: map 0
        const int seen = keys.size();
        W.map = keys(shift_key(L, v.reach_of(b), n_steps, W.flags.data()));
        if (W.map < seen) continue;
        Layout Ln;
        if ((rc = st.finish(Ln, why))) return rc;
        w.plan.phs.push_back(std::move(st.ph));
        w.plan.nl.push_back(Ln);
    }
    w.plan.map_id.resize(B);
    for (int b = 0; b < B; ++b) w.plan.map_id[b] = w.el[w.rep[b]].map;
    // one slot map for the batch when it agrees (the shared layout stays shared), else the elements'
    // own: per-element layouts, which need per-element references
    w.agree = !elem && w.plan.phs.size() == 1;
    if (!w.agree && B > 1 && v.Bref == 1) {
        why = "elements disagree on a contact change, which takes per-element layouts "
              "and per-element references (ref_per_element = 1)";
        return HSDDP_ERR_UNSUPPORTED;
    }
    w.flags.assign(n_steps, 0);
    for (int b = 0; b < B; ++b)
        if (w.rep[b] == b)
            for (int j = 0; j < n_steps; ++j) w.flags[j] |= w.el[b].flags[j];
    return HSDDP_OK;
}

void advance_rows(const HorizonView &v, const AdvanceWalk &w, int P, float plan_duration, float dt_mpc,
                  std::vector<int> &contacts, std::vector<double> &durations)
{
    const int B = v.B, P0 = v.P;
    contacts.assign((size_t)B * (P + 1) * 4, 0);
    durations.assign((size_t)B * P * 4, 0.0);
    for (int b = 0; b < B; ++b) {
        const AdvanceWalk::Element &W = w.el[w.rep[b]];
        const std::vector<ShiftPhase> &ph = w.plan.phs[W.map];
        const int Pb = (int)ph.size();
        for (int i = 0; i < Pb; ++i) {
            const int *cv = phase_contact(v, w, b, ph[i]);
            const double *dv = phase_duration(v, w, b, ph[i]);
            for (int l = 0; l < 4; ++l) {
                contacts[((size_t)b * (P + 1) + i) * 4 + l] = cv[l];
                durations[((size_t)b * P + i) * 4 + l] = dv[l];
            }
        }
        for (int l = 0; l < 4; ++l)
            contacts[((size_t)b * (P + 1) + Pb) * 4 + l] =
                W.next_kind == 0 ? v.contacts[((size_t)b * (P0 + 1) + W.P_old) * 4 + l]
                : W.next_kind == 1 ? window_sample(v, w.wsj[W.next_step], b, rel_at(w, b, W.next_step)).contact[l]
                                   : window_sample(v, w.wsj[W.next_step], b, plan_duration + dt_mpc).contact[l];
    }
}

// ---- hsddp_restart_elements ------------------------------------------------------------------------
std::vector<int> listed_elements(const int *mask, int B)
{
    std::vector<int> list;
    for (int b = 0; b < B; ++b)
        if (mask[b]) list.push_back(b);
    return list;
}

void put_restart_rows(const RestartPlan &plan, int P, int *contacts, double *durations)
{
    std::fill_n(contacts, (P + 1) * 4, 0);
    std::fill_n(durations, P * 4, 0.0);
    std::copy_n(plan.contacts, (plan.L.P + 1) * 4, contacts);
    std::copy_n(plan.durations, plan.L.P * 4, durations);
}

namespace {
// The batch's side of the listed elements taking the layouts, rows and reach flags of r.plans /
// r.reach_in, window starts start[m] and clocks clock[m].  fresh: new problems (a restart: no phase
// at its end, the clocks at 0, the slot maps of the new references); else elements that arrive as
// they stood elsewhere (hsddp_copy_elements / hsddp_import_elements).
int finish_batch(const HorizonView &v, const std::vector<int> &list, const int *start, const float *clock, bool fresh,
                 RestartBatch &r, std::string &why);
}  // namespace

int plan_restart_batch(const HorizonView &v, const std::vector<int> &list, const int *window_start,
                       float plan_duration, float dt_mpc, RestartBatch &r, std::string &why)
{
    const int n = (int)list.size();
    r = RestartBatch{};
    r.plans.resize(n);
    std::vector<int> start(n);
    for (int m = 0; m < n; ++m) {
        if (v.Bref == 1 && window_start[list[m]] != window_start[0]) {
            why = "shared references hold one window: every window start must be the same";
            return HSDDP_ERR_UNSUPPORTED;
        }
        if (int rc = plan_restart(v.table, v.ref_n, window_start[list[m]], v.win_len, v.ref_dt, plan_duration,
                                  v.dt_sim, dt_mpc, v.Kc, r.plans[m], why))
            return rc;
        start[m] = window_start[list[m]];
    }
    r.reach_in.assign((size_t)n * MAXP, 0);
    const std::vector<float> clock(n, 0.f);
    return finish_batch(v, list, start.data(), clock.data(), true, r, why);
}

void export_element(const HorizonView &v, int b, ElementImport &out)
{
    out = ElementImport{};
    const Layout &L = v.layout(b);
    out.L = L;
    std::copy_n(v.reach_of(b), L.P, out.reach);
    std::copy_n(&v.contacts[(size_t)b * (v.P + 1) * 4], (L.P + 1) * 4, out.contacts);
    if (v.durations) std::copy_n(&v.durations[(size_t)b * v.P * 4], L.P * 4, out.durations);
    out.win_start = v.win_start ? v.win_start[v.Bref == 1 ? 0 : b] : 0;
    out.clock = v.t_el ? v.t_el[b] : v.t_cur;
    out.has_terrain = v.terrain ? 1 : 0;
    if (v.terrain) std::copy_n(&v.terrain[(size_t)b * v.P * 2], L.P * 2, out.terrain);
    out.has_weights = v.weights ? 1 : 0;
    if (v.weights) std::copy_n(&v.weights[(size_t)b * NW], NW, out.weights);
}

void export_overrides(const HorizonView &v, int b, PhaseOverrides &out)
{
    const Layout &L = v.layout(b);
    std::memset(&out, 0, sizeof out);
    if (!v.pw_set) return;
    put_phase_weight_rows(&v.pw_set[(size_t)b * v.P], &v.pw[(size_t)b * v.P * NW], L.P, MAXP, out.set, out.rows);
    for (int i = 0; i < L.P; ++i) out.has |= out.set[i];
}

int plan_import_batch(const HorizonView &v, const std::vector<int> &list, const ElementImport *in, RestartBatch &r,
                      std::string &why)
{
    const int n = (int)list.size();
    r = RestartBatch{};
    r.plans.resize(n);
    r.reach_in.assign((size_t)n * MAXP, 0);
    std::vector<int> start(n), seen(v.B, 0);
    std::vector<float> clock(n);
    for (int m = 0; m < n; ++m) {
        if (list[m] < 0 || list[m] >= v.B) { why = "element index out of range"; return HSDDP_ERR_ARG; }
        if (seen[list[m]]++) { why = "a destination element is named twice"; return HSDDP_ERR_ARG; }
        const Layout &L = in[m].L;
        Layout chk;
        if (L.P < 1 || L.P > MAXP || build_layout(L.P, L.N, L.ss, chk, why) || std::memcmp(&chk, &L, sizeof(Layout)) ||
            control_slots(L) != v.Kc) {
            why = "an element's layout is not one of the handle's Kc control slots";
            return HSDDP_ERR_ARG;
        }
        r.plans[m].L = L;
        std::copy_n(in[m].contacts, (MAXP + 1) * 4, r.plans[m].contacts);
        std::copy_n(in[m].durations, MAXP * 4, r.plans[m].durations);
        for (int i = 0; i < L.P; ++i) r.reach_in[(size_t)m * MAXP + i] = in[m].reach[i] ? 1 : 0;
        start[m] = in[m].win_start;
        clock[m] = in[m].clock;
    }
    return finish_batch(v, list, start.data(), clock.data(), false, r, why);
}

namespace {
int finish_batch(const HorizonView &v, const std::vector<int> &list, const int *start, const float *clock, bool fresh,
                 RestartBatch &r, std::string &why)
{
    const int B = v.B, n = (int)list.size();
    const bool elem = v.lays != nullptr;
    r.all = n == B;
    auto reach_in = [&](int m) { return &r.reach_in[(size_t)m * MAXP]; };
    // The batch's largest P and S after the restart (the strides of the per-phase and per-slot
    // buffers).  Unlisted elements keep theirs, so the old strides stand unless a new layout exceeds
    // them or a listed element alone held them; only then is every element looked at.
    std::vector<int> listed(B, -1);
    for (int m = 0; m < n; ++m) listed[list[m]] = m;
    bool held = false;  // a listed element's old layout has the batch's largest P or S
    for (int m = 0; m < n; ++m) {
        r.Pn = std::max(r.Pn, r.plans[m].L.P);
        r.Sn = std::max(r.Sn, r.plans[m].L.S);
        const Layout &Lo = v.layout(list[m]);
        held = held || Lo.P == v.P || Lo.S == v.S;
    }
    if (!r.all) {
        if (!elem || !held || (r.Pn >= v.P && r.Sn >= v.S)) {
            r.Pn = std::max(r.Pn, v.P);
            r.Sn = std::max(r.Sn, v.S);
        } else {
            for (int b = 0; b < B; ++b)
                if (listed[b] < 0) {
                    r.Pn = std::max(r.Pn, v.lays[b].P);
                    r.Sn = std::max(r.Sn, v.lays[b].S);
                }
        }
    }
    if ((size_t)r.Sn > v.S_cap) {
        why = fresh ? "restarted layout exceeds the handle's capacity" : "an element's layout exceeds the handle's capacity";
        return HSDDP_ERR_ARG;
    }
    // one layout for the batch stays (or becomes) the shared one: every element listed, onto one
    // layout with one set of reach flags (a restart's: none), or some elements of a shared-layout
    // batch onto that layout with its flags.  (Elements with per-element layouts that come to agree
    // stay per element.)
    r.one = true;
    for (int m = 1; m < n && r.one; ++m)
        r.one = !std::memcmp(&r.plans[m].L, &r.plans[0].L, sizeof(Layout)) && std::equal(reach_in(m), reach_in(m) + MAXP, reach_in(0));
    if (!r.all)
        r.one = r.one && !elem && !std::memcmp(&r.plans[0].L, v.shared, sizeof(Layout)) &&
                std::equal(v.reach, v.reach + v.shared->P, reach_in(0));
    r.restride = r.Pn != v.P || r.Sn != v.S;
    // in place: the strides stand and the layouts are per element already, so the listed elements'
    // layout records, sweep pairs and table rows are patched and nothing of size B is built
    r.in_place = elem && !r.restride && !r.all;
    const int P = r.Pn;
    if (r.restride) {
        // the other elements' rows to the new strides: a shift of no steps (identity maps; the listed
        // elements' rows come out zero and are written by the restart)
        ShiftPlan &plan = r.stride_plan;
        plan.map_id.assign(B, 0);
        Interner keys;
        for (int b = 0; b < B; ++b) {
            const bool is = listed[b] >= 0;
            const Layout &L = is ? r.plans[listed[b]].L : v.layout(b);
            std::vector<int> key = !is ? shift_key(L, v.reach_of(b), 0, nullptr)
                                   : fresh ? layout_key(L, false) : shift_key(L, reach_in(listed[b]), 0, nullptr);
            key.push_back(is ? -2 : -3);
            const int seen = keys.size();
            plan.map_id[b] = keys(std::move(key));
            if (plan.map_id[b] < seen) continue;
            std::vector<ShiftPhase> ph;
            if (is) {
                for (int i = 0; i < L.P; ++i) {
                    ShiftPhase f;
                    f.N = L.N[i]; f.ss = L.ss[i]; f.reach = reach_in(listed[b])[i];
                    f.xs.assign(f.N + 1, -1); f.us.assign(f.N, -1); f.rs.assign(f.N, -1);
                    ph.push_back(f);
                }
            } else {
                ph = PhaseStepper(L, v.reach_of(b)).ph;
            }
            plan.phs.push_back(std::move(ph));
            plan.nl.push_back(L);
        }
        // contact rows [B][P + 1][4] and durations [B][P][4] at the new stride
        r.contacts.assign((size_t)B * (P + 1) * 4, 0);
        r.durations.assign((size_t)B * P * 4, 0.0);
        for (int b = 0; b < B; ++b) {
            int *c = &r.contacts[(size_t)b * (P + 1) * 4];
            double *d = &r.durations[(size_t)b * P * 4];
            if (listed[b] >= 0) {
                put_restart_rows(r.plans[listed[b]], P, c, d);
            } else {
                const int Pb = v.layout(b).P;
                std::copy_n(&v.contacts[(size_t)b * (v.P + 1) * 4], (Pb + 1) * 4, c);
                if (v.durations) std::copy_n(&v.durations[(size_t)b * v.P * 4], Pb * 4, d);
            }
        }
    } else if (!r.one && !r.in_place) {  // every element's layout and reach flags after the restart
        r.lays.resize(B);
        r.reach.assign((size_t)B * MAXP, 0);
        for (int b = 0; b < B; ++b) {
            if (listed[b] >= 0) {
                r.lays[b] = r.plans[listed[b]].L;
                std::copy_n(reach_in(listed[b]), MAXP, &r.reach[(size_t)b * MAXP]);
                continue;
            }
            r.lays[b] = v.layout(b);
            std::copy(v.reach_of(b), v.reach_of(b) + r.lays[b].P, &r.reach[(size_t)b * MAXP]);
        }
    }
    // the device rows of the listed elements: contact rows, slot maps (one per distinct new layout)
    r.rows.assign((size_t)n * (P + 1) * 4, 0);
    r.map_id.resize(n);
    r.start.resize(n);
    for (int m = 0; m < n; ++m) {
        std::copy_n(r.plans[m].contacts, (r.plans[m].L.P + 1) * 4, &r.rows[(size_t)m * (P + 1) * 4]);
        if (fresh) r.map_id[m] = r.slots.add(r.plans[m].L, nullptr, v.dt_sim, v.ref_dt, v.win_len - 1, r.Sn);
        r.start[m] = start[m];
    }
    if (v.win_start) {
        r.win_start.assign(v.win_start, v.win_start + v.Bref);
        for (int m = 0; m < n; ++m) r.win_start[v.Bref == 1 ? 0 : list[m]] = start[m];
    }
    // the clocks: QuadReference's t_cur restarts for the elements of a restart; an element that
    // arrives keeps its own, and the batch keeps one clock while every element agrees with it
    bool same = true;
    for (int m = 1; m < n; ++m) same = same && clock[m] == clock[0];
    r.t_cur = r.all && same ? clock[0] : v.t_cur;
    const bool shared = r.all ? same : !fresh && !v.t_el && same && clock[0] == v.t_cur;
    if (!shared) {
        r.t_el = v.t_el ? std::vector<float>(v.t_el, v.t_el + B) : std::vector<float>(B, v.t_cur);
        for (int m = 0; m < n; ++m) r.t_el[list[m]] = clock[m];
    }
    return HSDDP_OK;
}
}  // namespace

// ---- sweep pairs -----------------------------------------------------------------------------------
namespace {
// the n elements which[0..n) (null: 0..n) in groups of equal layout, the groups in key order
std::vector<std::vector<int>> layout_groups(const Layout *lays, const int *which, int n)
{
    Interner keys;
    std::vector<std::vector<int>> members;
    for (int j = 0; j < n; ++j) {
        const int b = which ? which[j] : j;
        const size_t q = keys(layout_key(lays[b], true));
        if (q == members.size()) members.emplace_back();
        members[q].push_back(b);
    }
    std::vector<std::vector<int>> groups;
    for (const auto &kv : keys.ids) groups.push_back(std::move(members[kv.second]));
    return groups;
}
}  // namespace

std::vector<int> pair_layouts(const std::vector<Layout> &lays)
{
    std::vector<int> pairs;
    for (const std::vector<int> &g : layout_groups(lays.data(), nullptr, (int)lays.size()))
        for (size_t j = 0; j < g.size(); j += 2) {
            pairs.push_back(g[j]);
            pairs.push_back(j + 1 < g.size() ? g[j + 1] : -1);
        }
    return pairs;
}

std::vector<int> patch_pairs(std::vector<int> &pr, std::vector<int> &of, int &n_pairs, const Layout *lays,
                             const std::vector<int> &list)
{
    int np = n_pairs;
    std::vector<int> freed, touched;
    for (int b : list) {
        const int q = of[b], partner = pr[2 * q] == b ? pr[2 * q + 1] : pr[2 * q];
        pr[2 * q] = partner;
        pr[2 * q + 1] = -1;
        if (partner < 0) freed.push_back(q);
        else touched.push_back(q);
        of[b] = -1;
    }
    for (const std::vector<int> &g : layout_groups(lays, list.data(), (int)list.size()))
        for (size_t j = 0; j < g.size(); j += 2) {
            int q;
            if (!freed.empty()) { q = freed.back(); freed.pop_back(); }
            else q = np++;
            if ((size_t)2 * q + 1 >= pr.size()) pr.resize((size_t)2 * q + 2, -1);
            pr[2 * q] = g[j];
            pr[2 * q + 1] = j + 1 < g.size() ? g[j + 1] : -1;
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
    n_pairs = np;
    return touched;
}

}  // namespace hsddp
