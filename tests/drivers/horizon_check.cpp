// horizon_check — the host bookkeeping of hsddp_advance and hsddp_restart_elements
// (hkd-mpc_amd/csrc/hsddp_phases.cpp: walk_advance, advance_rows, plan_restart_batch, flatten_shift,
// plan_refs, pair_layouts, patch_pairs) on a small batch's host state, from stdin, built from that
// source alone (no GPU, no product library): tests/test_horizon_host.py compares every element with
// the oracle's ProblemTracker.  The state below is the handle's host fields, and advance() / restart()
// commit a plan to it as hsddp_horizon.cpp's entry points do, minus the device.
//
// in:  "n dt_ref win_len plan_duration dt_sim dt_mpc Kc S_cap", then n lines "c0 c1 c2 c3 d0 d1 d2 d3"
//      (a sample's contact and status_dur), then "B Bref" and B window starts (every element is
//      started by plan_restart there), then commands:
//        advance <n_steps> | restart <k> <b> <start> ... | alter <b> <row> <leg> <value> | state
// out: per command "ok ..." or "refused <code> <text>"; state: one "batch" line and B "el" lines
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hsddp.h"
#include "../../hkd-mpc_amd/csrc/hsddp_phases.h"

using namespace hsddp;

namespace {

struct State {
    int B = 0, Bref = 1, Kc = 0, P = 0, S = 0, n_pairs = 0, win_len = 0;
    size_t S_cap = 0;
    float ref_dt = 0, dt_sim = 0, t_cur = 0;
    Layout shared{};
    std::vector<Layout> lays;
    std::vector<int> reach_end, reach_el, contacts, win_start, pairs, pair_of;
    std::vector<double> durations;
    std::vector<float> t_el;
    std::vector<hsddp_quad_state> table;

    HorizonView view() const
    {
        HorizonView v{};
        v.B = B; v.Bref = Bref; v.Kc = Kc; v.P = P; v.S = S;
        v.S_cap = S_cap;
        v.shared = &shared;
        v.lays = lays.empty() ? nullptr : lays.data();
        v.reach = v.lays ? reach_el.data() : reach_end.data();
        v.contacts = contacts.data(); v.durations = durations.data();
        v.table = table.data(); v.ref_n = (int)table.size(); v.ref_dt = ref_dt;
        v.win_start = win_start.data(); v.win_len = win_len; v.dt_sim = dt_sim;
        v.t_cur = t_cur;
        v.t_el = t_el.empty() ? nullptr : t_el.data();
        return v;
    }
    void adopt_shared(const Layout &L, const int *reach)
    {
        shared = L; P = L.P; S = L.S;
        lays.clear(); reach_el.clear(); pairs.clear(); pair_of.clear(); n_pairs = 0;
        reach_end.assign(reach, reach + L.P);
    }
    void set_layouts(const std::vector<Layout> &ls)
    {
        lays = ls;
        P = S = 0;
        for (const Layout &L : ls) { P = std::max(P, L.P); S = std::max(S, L.S); }
        pairs = pair_layouts(ls);
        n_pairs = (int)pairs.size() / 2;
        pair_of.assign(B, -1);
        for (size_t q = 0; q < pairs.size(); ++q)
            if (pairs[q] >= 0) pair_of[pairs[q]] = (int)(q / 2);
    }
};

template <typename T>
void csv(const char *name, const T *v, size_t n, const char *fmt)
{
    std::printf(" %s=", name);
    for (size_t i = 0; i < n; ++i) { std::printf(fmt, v[i]); if (i + 1 < n) std::printf(","); }
}

int refused(int rc, const std::string &why)
{
    std::printf("refused %d %s\n", rc, why.c_str());
    return rc;
}

// shift_apply's host side: the capacity check, then the new layouts
int apply_shift(State &st, const ShiftPlan &plan, std::string &why)
{
    ShiftMaps m;
    if (int rc = flatten_shift(plan, st.Kc, st.S_cap, m, why)) return rc;
    if (plan.phs.size() == 1) {
        int reach[MAXP];
        plan.reach(0, reach);
        st.adopt_shared(plan.nl[0], reach);
    } else {
        std::vector<Layout> lays;
        std::vector<int> reach;
        shifted_layouts(plan, lays, reach);
        st.set_layouts(lays);
        st.reach_el.swap(reach);
    }
    return HSDDP_OK;
}

void advance(State &st, int n_steps, float plan_duration, float dt_mpc)
{
    const HorizonView v = st.view();
    AdvanceWalk w;
    std::string why;
    if (int rc = walk_advance(v, n_steps, plan_duration, w, why)) { refused(rc, why); return; }
    if (int rc = apply_shift(st, w.plan, why)) { refused(rc, why); return; }
    std::vector<int> contacts;
    std::vector<double> dur;
    advance_rows(v, w, st.P, plan_duration, dt_mpc, contacts, dur);
    st.contacts.swap(contacts);
    st.durations.swap(dur);
    st.win_start = w.ws;
    if (st.t_el.empty()) st.t_cur = w.t_cur[0];
    else st.t_el = w.t_cur;
    std::printf("ok maps=%d agree=%d", (int)w.plan.phs.size(), (int)w.agree);
    csv("or", w.flags.data(), w.flags.size(), "%d");
    for (int b = 0; b < st.B; ++b) {
        const std::vector<int> &f = w.el[w.rep[b]].flags;
        csv("f", f.data(), f.size(), "%d");
    }
    std::printf("\n");
}

void restart(State &st, const std::vector<int> &mask, const std::vector<int> &ws, float plan_duration, float dt_mpc)
{
    const std::vector<int> list = listed_elements(mask.data(), st.B);
    const int n = (int)list.size();
    if (n == 0) { std::printf("ok none\n"); return; }
    if (n != st.B && st.Bref == 1) { refused(HSDDP_ERR_UNSUPPORTED, "shared references"); return; }
    RestartBatch r;
    std::string why;
    if (int rc = plan_restart_batch(st.view(), list, ws.data(), plan_duration, dt_mpc, r, why)) { refused(rc, why); return; }
    if (r.restride)
        if (int rc = apply_shift(st, r.stride_plan, why)) { refused(rc, why); return; }
    std::vector<int> touched;
    if (r.one) {
        const int none[MAXP] = {0};
        st.adopt_shared(r.plans[0].L, none);
    } else if (r.in_place) {
        for (int m = 0; m < n; ++m) {
            st.lays[list[m]] = r.plans[m].L;
            std::fill_n(&st.reach_el[(size_t)list[m] * MAXP], MAXP, 0);
        }
        touched = patch_pairs(st.pairs, st.pair_of, st.n_pairs, st.lays.data(), list);
    } else if (!r.restride) {
        st.set_layouts(r.lays);
        st.reach_el.swap(r.reach);
    }
    if (r.restride) {
        st.contacts.swap(r.contacts);
        st.durations.swap(r.durations);
    } else {
        for (int m = 0; m < n; ++m)
            put_restart_rows(r.plans[m], st.P, &st.contacts[(size_t)list[m] * (st.P + 1) * 4],
                             &st.durations[(size_t)list[m] * st.P * 4]);
    }
    st.win_start = r.win_start;
    if (r.all) st.t_cur = 0;
    st.t_el.swap(r.t_el);
    std::printf("ok one=%d in_place=%d restride=%d P=%d S=%d strideP=%d strideS=%d", (int)r.one, (int)r.in_place,
                (int)r.restride, r.Pn, r.Sn, st.P, st.S);
    csv("touched", touched.data(), touched.size(), "%d");
    csv("rows", r.rows.data(), r.rows.size(), "%d");
    csv("map_id", r.map_id.data(), r.map_id.size(), "%d");
    csv("start", r.start.data(), r.start.size(), "%d");
    csv("idx", r.slots.idx.data(), r.slots.idx.size(), "%d");
    std::printf("\n");
}

void print_state(const State &st)
{
    const HorizonView v = st.view();
    std::printf("batch elem=%d P=%d S=%d n_pairs=%d", (int)!st.lays.empty(), st.P, st.S, st.n_pairs);
    csv("pairs", st.pairs.data(), st.pairs.size(), "%d");
    csv("pair_of", st.pair_of.data(), st.pair_of.size(), "%d");
    const std::vector<int> fresh = st.lays.empty() ? std::vector<int>() : pair_layouts(st.lays);
    csv("fresh", fresh.data(), fresh.size(), "%d");
    RefPlan rp;  // the slot maps hsddp_advance's references are built with
    plan_refs(v, st.win_start.data(), st.win_len, nullptr, st.dt_sim, false, rp);
    std::printf(" maps=%d\n", (int)(rp.idx.size() / st.S));
    for (int b = 0; b < st.B; ++b) {
        const Layout &L = v.layout(b);
        std::printf("el %d", b);
        csv("N", L.N, L.P, "%d");
        csv("ss", L.ss, L.P, "%d");
        csv("reach", v.reach_of(b), L.P, "%d");
        csv("rows", &st.contacts[(size_t)b * (st.P + 1) * 4], (size_t)(st.P + 1) * 4, "%d");
        csv("dur", &st.durations[(size_t)b * st.P * 4], (size_t)st.P * 4, "%.17g");
        const std::vector<int> key = layout_key(L, true);
        csv("key", key.data(), key.size(), "%d");
        csv("slots", &rp.idx[(size_t)(st.lays.empty() ? 0 : rp.map_id[b]) * st.S], st.S, "%d");
        std::printf(" ws=%d t=%.9g\n", st.win_start[st.Bref == 1 ? 0 : b], (double)(st.t_el.empty() ? st.t_cur : st.t_el[b]));
    }
}

}  // namespace

int main()
{
    State st;
    int n, S_cap;
    float plan, dt_mpc;
    if (std::scanf("%d %f %d %f %f %f %d %d", &n, &st.ref_dt, &st.win_len, &plan, &st.dt_sim, &dt_mpc, &st.Kc, &S_cap) != 8 || n < 1)
        return 2;
    st.S_cap = S_cap;
    st.table.assign(n, hsddp_quad_state{});
    for (auto &q : st.table)
        if (std::scanf("%d %d %d %d %lf %lf %lf %lf", &q.contact[0], &q.contact[1], &q.contact[2], &q.contact[3],
                       &q.status_dur[0], &q.status_dur[1], &q.status_dur[2], &q.status_dur[3]) != 8)
            return 2;
    if (std::scanf("%d %d", &st.B, &st.Bref) != 2 || st.B < 1 || (st.Bref != 1 && st.Bref != st.B)) return 2;
    // every element a new problem at its window start: one layout for the batch is the shared one
    std::vector<int> starts(st.B);
    std::vector<RestartPlan> plans(st.B);
    std::vector<Layout> lays(st.B);
    bool same = true;
    for (int b = 0; b < st.B; ++b) {
        std::string why;
        if (std::scanf("%d", &starts[b]) != 1) return 2;
        if (int rc = plan_restart(st.table.data(), n, starts[b], st.win_len, st.ref_dt, plan, st.dt_sim, dt_mpc, st.Kc,
                                  plans[b], why)) {
            refused(rc, why);
            return 0;
        }
        lays[b] = plans[b].L;
        same = same && !std::memcmp(&lays[b], &lays[0], sizeof(Layout));
    }
    if (st.Bref == 1 && (!same || std::count(starts.begin(), starts.end(), starts[0]) != st.B)) return 2;
    const int none[MAXP] = {0};
    if (same) st.adopt_shared(lays[0], none);
    else {
        st.set_layouts(lays);
        st.reach_el.assign((size_t)st.B * MAXP, 0);
    }
    st.contacts.assign((size_t)st.B * (st.P + 1) * 4, 0);
    st.durations.assign((size_t)st.B * st.P * 4, 0.0);
    for (int b = 0; b < st.B; ++b)
        put_restart_rows(plans[b], st.P, &st.contacts[(size_t)b * (st.P + 1) * 4], &st.durations[(size_t)b * st.P * 4]);
    st.win_start.assign(starts.begin(), starts.begin() + st.Bref);
    std::printf("ok start\n");
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        const std::string c = cmd;
        if (c == "advance") {
            int k;
            if (std::scanf("%d", &k) != 1) return 2;
            advance(st, k, plan, dt_mpc);
        } else if (c == "restart") {
            int k;
            if (std::scanf("%d", &k) != 1) return 2;
            std::vector<int> mask(st.B, 0), ws(st.B, 0);
            for (int j = 0; j < k; ++j) {
                int b, s;
                if (std::scanf("%d %d", &b, &s) != 2 || b < 0 || b >= st.B) return 2;
                mask[b] = 1;
                ws[b] = s;
            }
            if (st.Bref == 1 && k > 0) std::fill(ws.begin(), ws.end(), ws[std::find(mask.begin(), mask.end(), 1) - mask.begin()]);
            restart(st, mask, ws, plan, dt_mpc);
        } else if (c == "alter") {
            int b, i, l, val;
            if (std::scanf("%d %d %d %d", &b, &i, &l, &val) != 4 || b < 0 || b >= st.B || i < 0 || i > st.P || l < 0 || l > 3) return 2;
            st.contacts[((size_t)b * (st.P + 1) + i) * 4 + l] = val;
            std::printf("ok alter\n");
        } else if (c == "state") {
            print_state(st);
        } else {
            return 2;
        }
    }
    return 0;
}
