// elements_check — the host bookkeeping of hsddp_copy_elements / hsddp_import_elements
// (hkd-mpc_amd/csrc/hsddp_phases.cpp: export_element, plan_import_batch, patch_pairs) on a small
// batch's host state, from stdin, built from that source alone (no GPU, no product library):
// tests/test_elements_host.py compares the decisions and the committed state with a short
// restatement.  The state below is the handle's host fields, and import() commits a plan to it as
// hsddp_horizon.cpp's move_elements does, minus the device.
//
// in:  "Kc S_cap B elem shared_clock t_cur", then B lines "P N.. ss.. reach.. clock id" (elem 0: all
//      one layout, the shared one), then "n" and n lines "dst P N.. ss.. reach.. clock win_start id".
//      An element with tag `id` has contact rows c[i][l] = (id + i + l) & 1, durations
//      d[i][l] = id + i / 4 + l / 64 and (in the batch) window start 100 + id.
// out: "refused <code> <text>", or "ok ..." with the decisions, a "batch" line and B "el" lines
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
    int B = 0, Kc = 0, P = 0, S = 0, n_pairs = 0;
    size_t S_cap = 0;
    float t_cur = 0;
    Layout shared{};
    std::vector<Layout> lays;
    std::vector<int> reach_end, reach_el, contacts, win_start, pairs, pair_of;
    std::vector<double> durations;
    std::vector<float> t_el;

    HorizonView view() const
    {
        HorizonView v{};
        v.B = B; v.Bref = B; v.Kc = Kc; v.P = P; v.S = S;
        v.S_cap = S_cap;
        v.shared = &shared;
        v.lays = lays.empty() ? nullptr : lays.data();
        v.reach = v.lays ? reach_el.data() : reach_end.data();
        v.contacts = contacts.data(); v.durations = durations.data();
        v.win_start = win_start.data();
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

struct Elem {
    Layout L;
    int reach[MAXP] = {0};
    float clock = 0;
    int id = 0;
};

bool read_elem(Elem &e)
{
    int P, N[MAXP], ss[MAXP];
    if (std::scanf("%d", &P) != 1 || P < 1 || P > MAXP) return false;
    for (int i = 0; i < P; ++i) if (std::scanf("%d", &N[i]) != 1) return false;
    for (int i = 0; i < P; ++i) if (std::scanf("%d", &ss[i]) != 1) return false;
    for (int i = 0; i < P; ++i) if (std::scanf("%d", &e.reach[i]) != 1) return false;
    std::string why;
    return build_layout(P, N, ss, e.L, why) == HSDDP_OK;
}

void tag_rows(int id, int P, int *c, double *d)
{
    for (int i = 0; i <= P; ++i)
        for (int l = 0; l < 4; ++l) c[i * 4 + l] = (id + i + l) & 1;
    for (int i = 0; i < P; ++i)
        for (int l = 0; l < 4; ++l) d[i * 4 + l] = id + i / 4.0 + l / 64.0;
}

}  // namespace

int main()
{
    State st;
    int S_cap, elem, shared_clock;
    if (std::scanf("%d %d %d %d %d %f", &st.Kc, &S_cap, &st.B, &elem, &shared_clock, &st.t_cur) != 6 || st.B < 1) return 2;
    st.S_cap = S_cap;
    std::vector<Elem> els(st.B);
    for (Elem &e : els)
        if (!read_elem(e) || std::scanf("%f %d", &e.clock, &e.id) != 2) return 2;
    if (elem) {
        std::vector<Layout> lays;
        for (const Elem &e : els) lays.push_back(e.L);
        st.set_layouts(lays);
        st.reach_el.assign((size_t)st.B * MAXP, 0);
        for (int b = 0; b < st.B; ++b) std::copy_n(els[b].reach, MAXP, &st.reach_el[(size_t)b * MAXP]);
    } else {
        st.adopt_shared(els[0].L, els[0].reach);
    }
    st.contacts.assign((size_t)st.B * (st.P + 1) * 4, 0);
    st.durations.assign((size_t)st.B * st.P * 4, 0.0);
    for (int b = 0; b < st.B; ++b) {
        tag_rows(els[b].id, els[b].L.P, &st.contacts[(size_t)b * (st.P + 1) * 4], &st.durations[(size_t)b * st.P * 4]);
        st.win_start.push_back(100 + els[b].id);
        if (!shared_clock) st.t_el.push_back(els[b].clock);
    }
    int n;
    if (std::scanf("%d", &n) != 1 || n < 0) return 2;
    std::vector<int> list(n);
    std::vector<ElementImport> in(n);
    for (int m = 0; m < n; ++m) {
        Elem e;
        if (std::scanf("%d", &list[m]) != 1 || !read_elem(e)) return 2;
        ElementImport &q = in[m];
        q = ElementImport{};
        if (std::scanf("%f %d %d", &q.clock, &q.win_start, &e.id) != 3) return 2;
        q.L = e.L;
        std::copy_n(e.reach, MAXP, q.reach);
        tag_rows(e.id, e.L.P, q.contacts, q.durations);
    }
    // export_element gives back what an element was made of
    for (int b = 0; b < st.B; ++b) {
        ElementImport q;
        export_element(st.view(), b, q);
        ElementImport w{};
        w.L = els[b].L;
        std::copy_n(els[b].reach, els[b].L.P, w.reach);
        tag_rows(els[b].id, els[b].L.P, w.contacts, w.durations);
        if (std::memcmp(&q.L, &w.L, sizeof(Layout)) || std::memcmp(q.reach, w.reach, sizeof w.reach) ||
            std::memcmp(q.contacts, w.contacts, sizeof w.contacts) || std::memcmp(q.durations, w.durations, sizeof w.durations) ||
            q.win_start != 100 + els[b].id || q.clock != (shared_clock ? st.t_cur : els[b].clock)) {
            std::printf("export mismatch %d\n", b);
            return 0;
        }
    }
    RestartBatch r;
    std::string why;
    if (int rc = plan_import_batch(st.view(), list, in.data(), r, why)) {
        std::printf("refused %d %s\n", rc, why.c_str());
        return 0;
    }
    // commit, as move_elements does
    std::vector<int> touched;
    if (r.restride) {
        ShiftMaps maps;
        if (int rc = flatten_shift(r.stride_plan, st.Kc, st.S_cap, maps, why)) { std::printf("refused %d %s\n", rc, why.c_str()); return 0; }
        if (r.stride_plan.phs.size() == 1) {
            int reach[MAXP];
            r.stride_plan.reach(0, reach);
            st.adopt_shared(r.stride_plan.nl[0], reach);
        } else {
            std::vector<Layout> lays;
            std::vector<int> reach;
            shifted_layouts(r.stride_plan, lays, reach);
            st.set_layouts(lays);
            st.reach_el.swap(reach);
        }
    }
    if (r.one) {
        st.adopt_shared(r.plans[0].L, &r.reach_in[0]);
    } else if (r.in_place) {
        for (int m = 0; m < n; ++m) {
            st.lays[list[m]] = r.plans[m].L;
            std::copy_n(&r.reach_in[(size_t)m * MAXP], MAXP, &st.reach_el[(size_t)list[m] * MAXP]);
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
    st.t_cur = r.t_cur;
    st.t_el.swap(r.t_el);
    std::printf("ok one=%d in_place=%d restride=%d all=%d P=%d S=%d strideP=%d strideS=%d", (int)r.one, (int)r.in_place,
                (int)r.restride, (int)r.all, r.Pn, r.Sn, st.P, st.S);
    std::sort(touched.begin(), touched.end());
    touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
    csv("touched", touched.data(), touched.size(), "%d");
    std::printf("\nbatch elem=%d n_pairs=%d shared_clock=%d t_cur=%.9g", (int)!st.lays.empty(), st.n_pairs, (int)st.t_el.empty(),
                (double)st.t_cur);
    csv("pairs", st.pairs.data(), (size_t)2 * st.n_pairs, "%d");
    csv("pair_of", st.pair_of.data(), st.pair_of.size(), "%d");
    std::printf("\n");
    const HorizonView v = st.view();
    for (int b = 0; b < st.B; ++b) {
        const Layout &L = v.layout(b);
        std::printf("el %d", b);
        csv("N", L.N, L.P, "%d");
        csv("ss", L.ss, L.P, "%d");
        csv("reach", v.reach_of(b), L.P, "%d");
        csv("rows", &st.contacts[(size_t)b * (st.P + 1) * 4], (size_t)(st.P + 1) * 4, "%d");
        csv("dur", &st.durations[(size_t)b * st.P * 4], (size_t)st.P * 4, "%.17g");
        std::printf(" ws=%d t=%.9g\n", st.win_start[b], (double)(st.t_el.empty() ? st.t_cur : st.t_el[b]));
    }
    return 0;
}
