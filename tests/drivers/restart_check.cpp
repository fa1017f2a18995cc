// restart_check — the host bookkeeping of hsddp_restart_elements (hsddp::plan_restart,
// hkd-mpc_amd/csrc/hsddp_phases.cpp) from stdin, built from that source alone (no GPU, no product
// library): tests/test_restart_host.py compares it with the oracle's ProblemTracker.
//
// in:  "n dt_ref win_len plan_duration dt_sim dt_mpc Kc", then n lines "c0 c1 c2 c3 d0 d1 d2 d3"
//      (a sample's contact and status_dur), then one window start per line
// out: per start "ok <N,..> <ss,..> <contact rows 0..P, 4 each> <durations, 4 per phase>"
//      or "refused <code>"
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/hsddp.h"
#include "../../hkd-mpc_amd/csrc/hsddp_phases.h"

int main()
{
    int n, win_len, Kc;
    float dt_ref, plan, dt_sim, dt_mpc;
    if (std::scanf("%d %f %d %f %f %f %d", &n, &dt_ref, &win_len, &plan, &dt_sim, &dt_mpc, &Kc) != 7 || n < 1) return 2;
    std::vector<hsddp_quad_state> table(n, hsddp_quad_state{});
    for (auto &q : table)
        if (std::scanf("%d %d %d %d %lf %lf %lf %lf", &q.contact[0], &q.contact[1], &q.contact[2], &q.contact[3],
                       &q.status_dur[0], &q.status_dur[1], &q.status_dur[2], &q.status_dur[3]) != 8)
            return 2;
    int start;
    while (std::scanf("%d", &start) == 1) {
        hsddp::RestartPlan r;
        std::string why;
        const int rc = hsddp::plan_restart(table.data(), n, start, win_len, dt_ref, plan, dt_sim, dt_mpc, Kc, r, why);
        if (rc) {
            std::printf("refused %d\n", rc);
            continue;
        }
        const int P = r.L.P;
        std::printf("ok ");
        for (int i = 0; i < P; ++i) std::printf("%d%s", r.L.N[i], i + 1 < P ? "," : " ");
        for (int i = 0; i < P; ++i) std::printf("%d%s", r.L.ss[i], i + 1 < P ? "," : " ");
        for (int e = 0; e < (P + 1) * 4; ++e) std::printf("%d%s", r.contacts[e], e + 1 < (P + 1) * 4 ? "," : " ");
        for (int e = 0; e < P * 4; ++e) std::printf("%.17g%s", r.durations[e], e + 1 < P * 4 ? "," : "\n");
    }
    return 0;
}
