// terrain_facade — the C++ facade with per-phase terrain: GRFConstraint::set_friction_coefficient and
// TouchDownConstraint::update_ground_height called with a different value per phase.
//   terrain_facade host     describe() alone (no GPU): phases that differ are collected as per-phase
//                           terrain, phases that agree stay the handle's cparams, two touchdown
//                           constraints of one phase with different ground are still refused
//   terrain_facade device   MultiPhaseDDP::solve against the C ABI given describe()'s arrays and
//                           hsddp_set_terrain, over three ticks (each starting from the last one's
//                           trajectories and constraint parameters, the first phase shrinking as an
//                           MPC tick's does): everything solve() writes back — Xbar, Ubar, K, the
//                           working rows, the objects' ReB / AL parameters — and the command record
//                           (hsddp_extract_commands) byte for byte; without hsddp_set_terrain they differ
#include <array>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "../../hkd-mpc_amd/facade/hkd_trajopt.hpp"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            return 1;                                                         \
        }                                                                     \
    } while (0)

using Phase = SinglePhase<double, 24, 24, 0>;
using Arr = std::array<int, 4>;

namespace {

struct Built {
    std::shared_ptr<Phase> ph;
    std::shared_ptr<Trajectory<double, 24, 24, 0>> traj;
    std::shared_ptr<hkd::GRFConstraint> grf;
    std::vector<std::shared_ptr<hkd::TouchDownConstraint>> td;
    std::shared_ptr<hkd::TrackingCost> tc;
    std::shared_ptr<hkd::FootPlaceReg> fr;
    // the reference tables follow the horizon (N + 1 rows of the standing reference)
    void fit_references()
    {
        const int N = traj->horizon;
        tc->x_ref.assign(N + 1, tc->x_ref[0]);
        tc->u_ref.assign(N + 1, tc->u_ref[0]);
        fr->foot_ref.assign(N + 1, fr->foot_ref[0]);
    }
};

// one HKD phase of N knots on contact c towards cn, standing references
Built hkd_phase(int N, const Arr &c, const Arr &cn, double t0)
{
    Built b;
    b.ph = std::make_shared<Phase>();
    b.traj = std::make_shared<Trajectory<double, 24, 24, 0>>(0.01, N);
    b.ph->set_trajectory(b.traj);
    hkd::Dynamics d;
    hkd::DynamicsPartial dp;
    hkd::Resetmap rm;
    hkd::ResetmapPartial rmp;
    d.contact = dp.contact = rm.contact = rmp.contact = c;
    rm.next_contact = rmp.next_contact = cn;
    b.ph->set_dynamics(d);
    b.ph->set_dynamics_partial(dp);
    b.ph->set_resetmap(rm);
    b.ph->set_resetmap_partial(rmp);
    auto tc = b.tc = std::make_shared<hkd::TrackingCost>();
    auto fr = b.fr = std::make_shared<hkd::FootPlaceReg>();
    std::array<double, 24> x{};
    x[5] = 0.25;
    const double feet[12] = {.2, -.14, 0, .2, .14, 0, -.2, -.14, 0, -.2, .14, 0};
    std::array<double, 12> pf{};
    for (int j = 0; j < 12; ++j) { x[12 + j] = feet[j]; pf[j] = feet[j]; }
    std::array<double, 24> u{};
    for (int l = 0; l < 4; ++l) u[3 * l + 2] = c[l] ? 9.0 * 9.81 / (c[0] + c[1] + c[2] + c[3]) : 0.0;
    tc->x_ref.assign(N + 1, x);
    tc->u_ref.assign(N + 1, u);
    fr->foot_ref.assign(N + 1, pf);
    b.ph->add_cost(tc);
    b.ph->add_cost(fr);
    if (c[0] + c[1] + c[2] + c[3] > 0) {
        b.grf = std::make_shared<hkd::GRFConstraint>(c);
        b.grf->update_horizon_len(N);  // (as HKDProblem::create_problem_one_phase: pop_front / push_back move its rows)
        b.grf->create_data();
        REB_Param_Struct<double> reb;
        reb.delta = b.grf->cparams.grf_delta; reb.delta_min = b.grf->cparams.grf_delta_min; reb.eps = b.grf->cparams.grf_eps;
        b.grf->initialize_params(reb);
        b.ph->add_pathConstraint(b.grf);
    }
    Arr impact{};
    bool any = false;
    for (int l = 0; l < 4; ++l) { impact[l] = c[l] == 0 && cn[l] == 1; any = any || impact[l]; }
    if (any) {
        b.td.push_back(std::make_shared<hkd::TouchDownConstraint>(impact));
        b.td.back()->create_data();
        hsddp_constraint_params cp;
        hsddp_default_constraint_params(&cp);
        AL_Param_Struct<double> al;
        al.sigma = cp.td_sigma; al.lambda = cp.td_lambda; al.sigma_max = cp.td_sigma_max;
        b.td.back()->initialize_params(al);
        b.ph->add_terminalConstraint(b.td.back());
    }
    b.ph->set_time_offset(t0);
    b.ph->update_SS_config(N + 1);
    for (int k = 0; k <= N; ++k)
        for (int j = 0; j < 24; ++j) { b.traj->Xbar[k][j] = x[j]; b.traj->X[k][j] = x[j]; }
    return b;
}

const Arr A{{1, 0, 0, 1}}, B{{0, 1, 1, 0}};
const double MU[3] = {0.45, 0.8, 0.6}, GROUND[3] = {0.015, -0.02, 0.03};

// three trot phases of n0, 6, 6 knots with per-phase values (same: one value for all)
std::vector<Built> problem(int n0, bool same)
{
    std::vector<Built> p{hkd_phase(n0, A, B, 0.0), hkd_phase(6, B, A, 0.01 * n0), hkd_phase(6, A, B, 0.01 * (n0 + 6))};
    for (int i = 0; i < 3; ++i) {
        p[i].grf->set_friction_coefficient(same ? MU[0] : MU[i]);
        for (auto &t : p[i].td) t->update_ground_height(same ? GROUND[0] : GROUND[i]);
    }
    return p;
}

// one MPC tick's edit of the phases: the first phase loses a knot, the last one gains one (the
// values stay with their constraint objects)
void tick_phases(std::vector<Built> &p, int tick)
{
    p[0].ph->pop_front();
    p[2].ph->push_back_default();
    p[2].ph->update_SS_config(p[2].traj->horizon + 1);
    p[0].fit_references();
    p[2].fit_references();
    p[1].ph->set_time_offset(0.01 * (6 - tick));
    p[2].ph->set_time_offset(0.01 * (12 - tick));
}

void install(MultiPhaseDDP<double> &s, const std::vector<Built> &p)
{
    std::deque<std::shared_ptr<SinglePhaseBase<double>>> phases;
    for (const Built &b : p) phases.push_back(b.ph);
    s.set_multiPhaseProblem(phases);
    DVec<double> x0(24);
    for (int j = 0; j < 24; ++j) x0[j] = p[0].traj->Xbar[0][j];
    x0[3] += 0.01;
    s.set_initial_condition(x0);
}

int host_checks()
{
    hsddp_constraint_params cp0;
    hsddp_default_constraint_params(&cp0);
    {   // phases that differ: per-phase terrain, the handle-wide pair the library's default
        MultiPhaseDDP<double> s;
        auto p = problem(6, false);
        install(s, p);
        const auto pr = s.describe();
        CHECK(pr.mu.size() == 3 && pr.ground.size() == 3);
        for (int i = 0; i < 3; ++i) CHECK(pr.mu[i] == MU[i] && pr.ground[i] == GROUND[i]);
        CHECK(pr.desc.cparams.mu_fric == cp0.mu_fric && pr.desc.cparams.ground_height == cp0.ground_height);
    }
    {   // phases that agree: the handle's cparams, no terrain
        MultiPhaseDDP<double> s;
        auto p = problem(6, true);
        install(s, p);
        const auto pr = s.describe();
        CHECK(pr.mu.empty() && pr.ground.empty());
        CHECK(pr.desc.cparams.mu_fric == MU[0] && pr.desc.cparams.ground_height == GROUND[0]);
    }
    {   // two touchdown constraints of one phase with different ground: refused
        MultiPhaseDDP<double> s;
        auto p = problem(6, false);
        Arr impact{{0, 1, 1, 0}};
        auto extra = std::make_shared<hkd::TouchDownConstraint>(impact);
        extra->update_ground_height(GROUND[0] + 0.01);
        p[0].ph->add_terminalConstraint(extra);
        install(s, p);
        bool refused = false;
        try {
            s.describe();
        } catch (const std::exception &e) {
            refused = std::strstr(e.what(), "same phase") != nullptr;
        }
        CHECK(refused);
        extra->update_ground_height(GROUND[0]);  // the same ground: two constraints of the phase, accepted
        CHECK(s.describe().ground[0] == GROUND[0]);
    }
    {   // the phases move through the horizon: each keeps its pair
        MultiPhaseDDP<double> s;
        auto p = problem(6, false);
        for (int tick = 1; tick < 3; ++tick) {
            tick_phases(p, tick);
            install(s, p);
            const auto pr = s.describe();
            CHECK(pr.desc.horizons[0] == 6 - tick && pr.desc.horizons[2] == 6 + tick);
            for (int i = 0; i < 3; ++i) CHECK(pr.mu[i] == MU[i] && pr.ground[i] == GROUND[i]);
        }
    }
    {   // a differing delta_min is still refused
        MultiPhaseDDP<double> s;
        auto p = problem(6, false);
        p[1].grf->cparams.grf_delta_min *= 2;
        install(s, p);
        bool refused = false;
        try {
            s.describe();
        } catch (const std::exception &e) {
            refused = std::strstr(e.what(), "delta_min") != nullptr;
        }
        CHECK(refused);
    }
    std::printf("terrain_facade host ok\n");
    return 0;
}

#define ABI(call)                                                             \
    do {                                                                      \
        if ((call) != HSDDP_OK) {                                             \
            std::printf("FAILED %s: %s\n", #call, hsddp_last_error());        \
            return 1;                                                         \
        }                                                                     \
    } while (0)

// what a solve leaves for the caller and the next tick
struct Solved {
    std::vector<double> Xbar, Ubar, K, X, U, reb_delta, reb_eps, al_sigma, al_lambda;
    hsddp_mpc_command cmd;
};

int new_handle(const MultiPhaseDDP<double>::Problem &pr, const std::vector<double> &x0, const hsddp_options &o, hsddp_handle &h)
{
    hsddp_problem_desc desc = pr.desc;
    desc.batch = 1;
    ABI(hsddp_create(&desc, &h));
    ABI(hsddp_set_layout(h, desc.n_phases, desc.horizons, pr.shooting.data(), nullptr));
    ABI(hsddp_set_options(h, &o));
    ABI(hsddp_upload_problem(h, pr.contacts.data(), x0.data(), pr.ref_x.data(), pr.ref_u.data(), pr.ref_foot.data()));
    return 0;
}

// HKDMPCSolver::publish_mpc_cmd's record of the handle's trajectory (every byte written by the kernel)
int commands_of(hsddp_handle h, int tick, hsddp_mpc_command &cmd)
{
    std::memset(&cmd, 0, sizeof cmd);
    ABI(hsddp_extract_commands(h, 1, 0.01 * tick, 0.01, nullptr, 0, nullptr, 0, 0.f, &cmd));
    return 0;
}

// the C-ABI path on describe()'s arrays; terrain: with hsddp_set_terrain
int abi_solve(const MultiPhaseDDP<double>::Problem &pr, const std::vector<double> &x0, const hsddp_options &o, bool terrain,
              int tick, Solved &out)
{
    hsddp_handle h = nullptr;
    if (new_handle(pr, x0, o, h)) return 1;
    ABI(hsddp_upload_warm_start(h, pr.Xbar.data(), pr.Ubar.data(), pr.K.data()));
    ABI(hsddp_upload_constraint_params(h, pr.reb_delta.data(), pr.reb_eps.data(), pr.td_legs.data(), pr.al_sigma.data(),
                                       pr.al_lambda.data()));
    if (terrain) ABI(hsddp_set_terrain(h, pr.mu.data(), pr.ground.data()));
    ABI(hsddp_solve(h, nullptr));
    const size_t S = pr.S, Kc = pr.Kc;
    out.Xbar.assign(S * 24, 0.0); out.X.assign(S * 24, 0.0);
    out.Ubar.assign(Kc * 24, 0.0); out.U.assign(Kc * 24, 0.0);
    out.K.assign(Kc * 576, 0.0);
    out.reb_delta = pr.reb_delta; out.reb_eps = pr.reb_eps; out.al_sigma = pr.al_sigma; out.al_lambda = pr.al_lambda;
    ABI(hsddp_download_trajectory(h, out.Xbar.data(), out.Ubar.data(), out.K.data()));
    ABI(hsddp_download_working(h, out.X.data(), out.U.data(), nullptr, nullptr, nullptr));
    ABI(hsddp_download_constraint_params(h, out.reb_delta.data(), out.reb_eps.data(), nullptr, out.al_sigma.data(),
                                         out.al_lambda.data()));
    if (commands_of(h, tick, out.cmd)) return 1;
    hsddp_destroy(h);
    return 0;
}

bool same(const std::vector<double> &a, const std::vector<double> &b)
{
    return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(double));
}

int device_checks()
{
    HSDDP_OPTION opt;
    opt.max_AL_iter = 2;
    opt.max_DDP_iter = 2;
    const hsddp_options o = opt.to_c();
    MultiPhaseDDP<double> s;
    auto p = problem(6, false);
    for (int tick = 0; tick < 3; ++tick) {
        if (tick) tick_phases(p, tick);
        install(s, p);
        const auto pr = s.describe();
        CHECK(pr.mu.size() == 3 && pr.mu[1] == MU[1] && pr.ground[2] == GROUND[2]);
        std::vector<double> x0(24);
        for (int j = 0; j < 24; ++j) x0[j] = p[0].traj->Xbar[0][j];
        x0[3] += 0.01;
        Solved a, n;
        if (abi_solve(pr, x0, o, true, tick, a) || abi_solve(pr, x0, o, false, tick, n)) return 1;
        s.solve(opt);
        // everything solve() wrote back — the trajectories and gains, and the constraint objects' ReB /
        // AL parameters — as the next tick's describe() reads it, and the working rows
        const auto after = s.describe();
        CHECK(same(after.Xbar, a.Xbar) && same(after.Ubar, a.Ubar) && same(after.K, a.K));
        CHECK(same(after.reb_delta, a.reb_delta) && same(after.reb_eps, a.reb_eps));
        CHECK(same(after.al_sigma, a.al_sigma) && same(after.al_lambda, a.al_lambda));
        std::vector<double> Xw, Uw;
        for (const Built &b : p) {
            for (int k = 0; k <= b.traj->horizon; ++k)
                for (int j = 0; j < 24; ++j) Xw.push_back(b.traj->X[k][j]);
            for (int k = 0; k < b.traj->horizon; ++k)
                for (int j = 0; j < 24; ++j) Uw.push_back(b.traj->U[k][j]);
        }
        CHECK(same(Xw, a.X) && same(Uw, a.U));
        // the command record formed from what the facade wrote back: the same bytes as the C-ABI path's
        hsddp_handle h = nullptr;
        hsddp_mpc_command cmd;
        if (new_handle(pr, x0, o, h)) return 1;
        ABI(hsddp_upload_warm_start(h, after.Xbar.data(), after.Ubar.data(), after.K.data()));
        if (commands_of(h, tick, cmd)) return 1;
        hsddp_destroy(h);
        CHECK(!std::memcmp(&cmd, &a.cmd, sizeof cmd));
        // (the table is read: without hsddp_set_terrain the solve and its commands are others)
        CHECK(!same(after.Ubar, n.Ubar) && std::memcmp(&cmd, &n.cmd, sizeof cmd) != 0);
        std::printf("tick %d: facade == C ABI with hsddp_set_terrain\n", tick);
    }
    std::printf("terrain_facade device ok\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);  // (a crash keeps the lines before it)
    try {
        const std::string mode = argc > 1 ? argv[1] : "host";
        return mode == "device" ? device_checks() : host_checks();
    } catch (const std::exception &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
}
