// phase_weights_check — the host bookkeeping of the per-phase weight overrides
// (hsddp_set_phase_weights; hkd-mpc_amd/csrc/hsddp_phases.cpp: shift_phase_weights,
// put_phase_weight_rows, export_overrides) on a small batch's host state, from stdin, built from that
// source alone (no GPU, no product library): tests/test_phase_weights_host.py compares the flags and
// rows after every command with a short restatement.  The commands commit their plans to the state as
// hsddp_horizon.cpp's shift_apply, hsddp_restart_elements and move_elements do, minus the device.
//
// in:  "rows Kc S_cap B elem", then B lines "P N.. reach.." (elem 0: all one layout, the shared
//      one); or "table n dt_ref win_len plan_duration dt_sim dt_mpc Kc S_cap", n lines
//      "c0 c1 c2 c3 d0 d1 d2 d3" (a sample's contact and status_dur), "B" and B window starts (every
//      element started by plan_restart there, per-element references).  Phase i of element b starts
//      with an override where (b + i) % 3 != 0: the row whose field j is 100 b + i + (j + 1) / 64.
//      Then commands (the first two need the table):
//      "advance n"                                           hsddp_advance (walk_advance's plan)
//      "restart k" and k pairs "b start"                     hsddp_restart_elements (plan_restart_batch)
//      "shift n" and B lines of n contact-change flags       hsddp_shift_elements / hsddp_advance
//      "take n" and n lines "dst tag P N.. reach.."          an element arriving in slot dst
//          (hsddp_copy_elements / hsddp_import_elements) with overrides on its even phases, field j
//          of phase i at 5000 + 100 tag + i + (j + 1) / 64; tag < 0: without overrides
// out: after the start and after each command "state P=<stride> elem=<0|1>" and B lines
//      "el b N=.. reach=.. set=.. rows=first,last,.." (flag, and first and last field of the row, of
//      every phase of the stride; a row without a flag is zero), or "refused <code> <text>"
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
    int B = 0, Kc = 0, P = 0, S = 0, win_len = 0;
    size_t S_cap = 0;
    float ref_dt = 0, dt_sim = 0, t_cur = 0;
    Layout shared{};
    std::vector<Layout> lays;
    std::vector<int> reach_end, reach_el, contacts, win_start;
    std::vector<double> pw, durations;
    std::vector<int> pw_set;
    std::vector<float> t_el;
    std::vector<hsddp_quad_state> table;

    HorizonView view() const
    {
        HorizonView v{};
        v.B = B; v.Bref = B; v.Kc = Kc; v.P = P; v.S = S;
        v.S_cap = S_cap;
        v.shared = &shared;
        v.lays = lays.empty() ? nullptr : lays.data();
        v.reach = v.lays ? reach_el.data() : reach_end.data();
        v.contacts = contacts.data();
        v.durations = durations.empty() ? nullptr : durations.data();
        v.table = table.data(); v.ref_n = (int)table.size(); v.ref_dt = ref_dt;
        v.win_len = win_len; v.dt_sim = dt_sim;
        v.t_cur = t_cur;
        v.t_el = t_el.empty() ? nullptr : t_el.data();
        v.win_start = win_start.data();
        v.pw_set = pw_set.empty() ? nullptr : pw_set.data();
        v.pw = pw.empty() ? nullptr : pw.data();
        return v;
    }
    void adopt_shared(const Layout &L, const int *reach)
    {
        shared = L; P = L.P; S = L.S;
        lays.clear(); reach_el.clear();
        reach_end.assign(reach, reach + L.P);
    }
    void set_layouts(const std::vector<Layout> &ls, std::vector<int> &reach)
    {
        lays = ls;
        P = S = 0;
        for (const Layout &L : ls) { P = std::max(P, L.P); S = std::max(S, L.S); }
        reach_el.swap(reach);
    }
    // (the contact rows are not compared: zero rows at the current stride keep the view's reads in range)
    void restride_contacts() { contacts.assign((size_t)B * (P + 1) * 4, 0); }
    // a plan's layouts, as shift_apply installs them
    void install(const ShiftPlan &plan)
    {
        if (plan.phs.size() == 1) {
            int reach[MAXP];
            plan.reach(0, reach);
            adopt_shared(plan.nl[0], reach);
        } else {
            std::vector<Layout> ls;
            std::vector<int> reach;
            shifted_layouts(plan, ls, reach);
            set_layouts(ls, reach);
        }
    }
    void print() const
    {
        const HorizonView v = view();
        std::printf("state P=%d elem=%d\n", P, (int)!lays.empty());
        for (int b = 0; b < B; ++b) {
            const Layout &L = v.layout(b);
            std::printf("el %d N=", b);
            for (int i = 0; i < L.P; ++i) std::printf("%d%s", L.N[i], i + 1 < L.P ? "," : "");
            std::printf(" reach=");
            for (int i = 0; i < L.P; ++i) std::printf("%d%s", v.reach_of(b)[i], i + 1 < L.P ? "," : "");
            std::printf(" set=");
            for (int i = 0; i < P; ++i) std::printf("%d%s", pw_set[(size_t)b * P + i], i + 1 < P ? "," : "");
            std::printf(" rows=");
            for (int i = 0; i < P; ++i) {
                const double *r = &pw[((size_t)b * P + i) * NW];
                for (int j = 1; j + 1 < NW; ++j)  // (a row is whole: its fields differ by 1 / 64)
                    if (pw_set[(size_t)b * P + i] ? r[j] != r[0] + j / 64.0 : r[j] != 0.0) std::printf("torn");
                std::printf("%.17g,%.17g%s", r[0], r[NW - 1], i + 1 < P ? "," : "");
            }
            std::printf("\n");
        }
    }
};

bool read_layout(Layout &L, int *reach)
{
    int P, N[MAXP];
    if (std::scanf("%d", &P) != 1 || P < 1 || P > MAXP) return false;
    for (int i = 0; i < P; ++i) if (std::scanf("%d", &N[i]) != 1) return false;
    std::fill_n(reach, MAXP, 0);
    for (int i = 0; i < P; ++i) if (std::scanf("%d", &reach[i]) != 1) return false;
    std::string why;
    return build_layout(P, N, nullptr, L, why) == HSDDP_OK;
}

// the table, and every element a new problem at its window start (plan_restart)
bool read_table_batch(State &st, float &plan, float &dt_mpc)
{
    int n, S_cap;
    if (std::scanf("%d %f %d %f %f %f %d %d", &n, &st.ref_dt, &st.win_len, &plan, &st.dt_sim, &dt_mpc, &st.Kc, &S_cap) != 8 || n < 1)
        return false;
    st.S_cap = S_cap;
    st.table.assign(n, hsddp_quad_state{});
    for (auto &q : st.table)
        if (std::scanf("%d %d %d %d %lf %lf %lf %lf", &q.contact[0], &q.contact[1], &q.contact[2], &q.contact[3],
                       &q.status_dur[0], &q.status_dur[1], &q.status_dur[2], &q.status_dur[3]) != 8)
            return false;
    if (std::scanf("%d", &st.B) != 1 || st.B < 1) return false;
    std::vector<RestartPlan> plans(st.B);
    std::vector<Layout> lays(st.B);
    st.win_start.resize(st.B);
    for (int b = 0; b < st.B; ++b) {
        std::string why;
        if (std::scanf("%d", &st.win_start[b]) != 1 ||
            plan_restart(st.table.data(), n, st.win_start[b], st.win_len, st.ref_dt, plan, st.dt_sim, dt_mpc, st.Kc, plans[b], why))
            return false;
        lays[b] = plans[b].L;
    }
    std::vector<int> reach((size_t)st.B * MAXP, 0);
    st.set_layouts(lays, reach);
    st.contacts.assign((size_t)st.B * (st.P + 1) * 4, 0);
    st.durations.assign((size_t)st.B * st.P * 4, 0.0);
    for (int b = 0; b < st.B; ++b)
        put_restart_rows(plans[b], st.P, &st.contacts[(size_t)b * (st.P + 1) * 4], &st.durations[(size_t)b * st.P * 4]);
    return true;
}

// hsddp_advance's host side (advance_impl), with the overrides as shift_apply carries them
bool advance(State &st, int n_steps, float plan, float dt_mpc)
{
    const HorizonView v = st.view();
    AdvanceWalk w;
    ShiftMaps maps;
    std::string why;
    int rc = walk_advance(v, n_steps, plan, w, why);
    if (!rc) rc = flatten_shift(w.plan, st.Kc, st.S_cap, maps, why);
    if (rc) { std::printf("refused %d %s\n", rc, why.c_str()); return false; }
    std::vector<double> t;
    std::vector<int> f;
    shift_phase_weights(v, w.plan, maps.P_new, f, t);
    st.install(w.plan);
    st.pw.swap(t);
    st.pw_set.swap(f);
    std::vector<int> contacts;
    std::vector<double> dur;
    advance_rows(v, w, st.P, plan, dt_mpc, contacts, dur);  // (v: the old rows, which these vectors still hold)
    st.contacts.swap(contacts);
    st.durations.swap(dur);
    st.win_start = w.ws;
    if (st.t_el.empty()) st.t_cur = w.t_cur[0];
    else st.t_el = w.t_cur;
    return true;
}

// hsddp_restart_elements' host side, with the overrides: the restride pass carries the others',
// the restarted elements have none
bool restart(State &st, const std::vector<int> &mask, const std::vector<int> &ws, float plan, float dt_mpc)
{
    const std::vector<int> list = listed_elements(mask.data(), st.B);
    const int n = (int)list.size();
    RestartBatch r;
    std::string why;
    if (int rc = plan_restart_batch(st.view(), list, ws.data(), plan, dt_mpc, r, why)) { std::printf("refused %d %s\n", rc, why.c_str()); return false; }
    if (r.restride) {
        std::vector<double> t;
        std::vector<int> f;
        shift_phase_weights(st.view(), r.stride_plan, r.Pn, f, t);
        st.install(r.stride_plan);
        st.pw.swap(t);
        st.pw_set.swap(f);
    }
    if (r.one) {
        const int none[MAXP] = {0};
        st.adopt_shared(r.plans[0].L, none);
    } else if (r.in_place) {
        for (int m = 0; m < n; ++m) {
            st.lays[list[m]] = r.plans[m].L;
            std::fill_n(&st.reach_el[(size_t)list[m] * MAXP], MAXP, 0);
        }
    } else if (!r.restride) {
        st.set_layouts(r.lays, r.reach);
    }
    if (r.restride) {
        st.contacts.swap(r.contacts);
        st.durations.swap(r.durations);
    } else {
        for (int m = 0; m < n; ++m)
            put_restart_rows(r.plans[m], st.P, &st.contacts[(size_t)list[m] * (st.P + 1) * 4], &st.durations[(size_t)list[m] * st.P * 4]);
    }
    for (int m = 0; m < n; ++m)
        put_phase_weight_rows(nullptr, nullptr, 0, st.P, &st.pw_set[(size_t)list[m] * st.P], &st.pw[(size_t)list[m] * st.P * NW]);
    st.win_start = r.win_start;
    if (r.all) st.t_cur = 0;
    st.t_el.swap(r.t_el);
    return true;
}

}  // namespace

int main()
{
    State st;
    int S_cap, elem;
    char mode[16];
    float plan = 0, dt_mpc = 0;
    if (std::scanf("%15s", mode) != 1) return 2;
    const bool with_table = !std::strcmp(mode, "table");
    if (with_table) {
        if (!read_table_batch(st, plan, dt_mpc)) return 2;
    } else {
        if (std::scanf("%d %d %d %d", &st.Kc, &S_cap, &st.B, &elem) != 4 || st.B < 1) return 2;
        st.S_cap = S_cap;
        std::vector<Layout> ls(st.B);
        std::vector<int> reach((size_t)st.B * MAXP, 0);
        for (int b = 0; b < st.B; ++b)
            if (!read_layout(ls[b], &reach[(size_t)b * MAXP])) return 2;
        if (elem) st.set_layouts(ls, reach);
        else st.adopt_shared(ls[0], reach.data());
        st.restride_contacts();
        st.win_start.assign(st.B, 0);
    }
    st.pw_set.assign((size_t)st.B * st.P, 0);
    st.pw.assign((size_t)st.B * st.P * NW, 0.0);
    for (int b = 0; b < st.B; ++b) {
        std::vector<int> set(MAXP);
        std::vector<double> rows((size_t)MAXP * NW);
        for (int i = 0; i < MAXP; ++i) {
            set[i] = (b + i) % 3 != 0;
            for (int j = 0; j < NW; ++j) rows[(size_t)i * NW + j] = 100 * b + i + (j + 1) / 64.0;
        }
        put_phase_weight_rows(set.data(), rows.data(), st.view().layout(b).P, st.P, &st.pw_set[(size_t)b * st.P], &st.pw[(size_t)b * st.P * NW]);
    }
    st.print();
    char cmd[16];
    std::string why;
    while (std::scanf("%15s", cmd) == 1) {
        int n;
        if (std::scanf("%d", &n) != 1 || n < 0) return 2;
        if (with_table && !std::strcmp(cmd, "advance")) {
            if (!advance(st, n, plan, dt_mpc)) continue;
        } else if (with_table && !std::strcmp(cmd, "restart")) {
            std::vector<int> mask(st.B, 0), ws(st.B, 0);
            for (int j = 0; j < n; ++j) {
                int b, s0;
                if (std::scanf("%d %d", &b, &s0) != 2 || b < 0 || b >= st.B) return 2;
                mask[b] = 1;
                ws[b] = s0;
            }
            if (!restart(st, mask, ws, plan, dt_mpc)) continue;
        } else if (with_table) {
            return 2;  // (shift and take leave the table's rows behind)
        } else if (!std::strcmp(cmd, "shift")) {
            std::vector<int> cc((size_t)st.B * n);
            for (int &f : cc) if (std::scanf("%d", &f) != 1) return 2;
            ShiftPlan plan;
            ShiftMaps maps;
            int rc = plan_shift(st.view(), n, cc.data(), n, plan, why);
            if (!rc) rc = flatten_shift(plan, st.Kc, st.S_cap, maps, why);
            if (rc) { std::printf("refused %d %s\n", rc, why.c_str()); continue; }
            std::vector<double> t;
            std::vector<int> f;
            shift_phase_weights(st.view(), plan, maps.P_new, f, t);
            st.install(plan);
            st.pw.swap(t);
            st.pw_set.swap(f);
            st.restride_contacts();
        } else if (!std::strcmp(cmd, "take")) {
            std::vector<int> list(n);
            std::vector<ElementImport> in(n);
            std::vector<PhaseOverrides> ov(n);
            for (int m = 0; m < n; ++m) {
                int tag;
                ElementImport &q = in[m];
                q = ElementImport{};
                if (std::scanf("%d %d", &list[m], &tag) != 2 || !read_layout(q.L, q.reach)) return 2;
                PhaseOverrides &o = ov[m];
                o = PhaseOverrides{};
                o.has = tag >= 0;
                for (int i = 0; i < q.L.P && tag >= 0; i += 2) {
                    o.set[i] = 1;
                    for (int j = 0; j < NW; ++j) o.rows[(size_t)i * NW + j] = 5000 + 100 * tag + i + (j + 1) / 64.0;
                }
            }
            RestartBatch r;
            if (int rc = plan_import_batch(st.view(), list, in.data(), r, why)) { std::printf("refused %d %s\n", rc, why.c_str()); continue; }
            if (r.restride) {
                std::vector<double> t;
                std::vector<int> f;
                shift_phase_weights(st.view(), r.stride_plan, r.Pn, f, t);
                st.install(r.stride_plan);
                st.pw.swap(t);
                st.pw_set.swap(f);
            }
            if (r.one) {
                st.adopt_shared(r.plans[0].L, &r.reach_in[0]);
            } else if (r.in_place) {
                for (int m = 0; m < n; ++m) {
                    st.lays[list[m]] = r.plans[m].L;
                    std::copy_n(&r.reach_in[(size_t)m * MAXP], MAXP, &st.reach_el[(size_t)list[m] * MAXP]);
                }
            } else if (!r.restride) {
                st.set_layouts(r.lays, r.reach);
            }
            st.restride_contacts();
            for (int m = 0; m < n; ++m)
                put_phase_weight_rows(ov[m].has ? ov[m].set : nullptr, ov[m].rows, in[m].L.P, st.P,
                                      &st.pw_set[(size_t)list[m] * st.P], &st.pw[(size_t)list[m] * st.P * NW]);
            // what the arriving element's record would carry on, once in place
            for (int m = 0; m < n; ++m) {
                ElementImport q;
                PhaseOverrides o;
                export_element(st.view(), list[m], q);
                export_overrides(st.view(), list[m], o);
                bool ok = o.has == (ov[m].has && in[m].L.P > 0);
                for (int i = 0; i < q.L.P; ++i) {
                    ok = ok && o.set[i] == st.pw_set[(size_t)list[m] * st.P + i];
                    for (int j = 0; j < NW; ++j) ok = ok && o.rows[(size_t)i * NW + j] == st.pw[((size_t)list[m] * st.P + i) * NW + j];
                }
                for (int i = q.L.P; i < MAXP; ++i) ok = ok && !o.set[i];
                if (!ok) { std::printf("export mismatch %d\n", list[m]); return 0; }
            }
        } else {
            return 2;
        }
        st.print();
    }
    return 0;
}
