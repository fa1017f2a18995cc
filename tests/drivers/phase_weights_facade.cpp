// phase_weights_facade — the C++ facade with cost objects that differ from phase to phase, as
// HKDProblem::create_problem_one_phase builds one HKDTrackingCost and one HKDFootPlaceReg per phase.
//   phase_weights_facade host     describe() alone (no GPU): one weight row per phase, through the
//                                 hkd:: terms (their hsddp_hkd_weights) and through diagonals alone
//                                 (the reference classes' Q, R, Qf, Qfoot: the quotient rule per
//                                 phase); phases that agree give no overrides; a field a phase's
//                                 contact masks out is the handle-wide one; qJ weight on a stance
//                                 leg is still refused, and so are differing phases while
//                                 per_phase_weights is off (the default)
//   phase_weights_facade device   MultiPhaseDDP::solve of such a problem, both ways, against the C ABI
//                                 given describe()'s arrays and hsddp_set_phase_weights, over three
//                                 ticks (the first phase shrinking as an MPC tick's does): everything
//                                 solve() writes back, byte for byte; without the overrides they differ
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
// hkd:: terms whose weights reach describe() as diagonals only, as the reference's HKDTrackingCost /
// HKDFootPlaceReg give theirs (Q, R, Qf, Qfoot): the quotient rule applies, phase by phase
struct DiagTracking : hkd::TrackingCost {
    void device_spec(hsddp_facade::CostSpec &spec, const int *c) const override
    {
        hkd::TrackingCost::device_spec(spec, c);
        spec.exact = nullptr;
    }
};
struct DiagFoot : hkd::FootPlaceReg {
    void device_spec(hsddp_facade::CostSpec &spec, const int *c) const override
    {
        hkd::FootPlaceReg::device_spec(spec, c);
        spec.exact = nullptr;
    }
};

// qJ weight on the stance legs: no row of HKD weights gives it
struct StanceQJ : DiagTracking {
    void device_spec(hsddp_facade::CostSpec &spec, const int *c) const override
    {
        DiagTracking::device_spec(spec, c);
        for (int l = 0; l < 4; ++l)
            if (c[l]) spec.q[12 + 3 * l] = 0.3;
    }
};

// (diag 2: StanceQJ as the tracking term)
Built hkd_phase(int N, const Arr &c, const Arr &cn, double t0, int diag)
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
    auto tc = b.tc = diag == 2 ? std::make_shared<StanceQJ>() : diag ? std::make_shared<DiagTracking>() : std::make_shared<hkd::TrackingCost>();
    auto fr = b.fr = diag ? std::make_shared<DiagFoot>() : std::make_shared<hkd::FootPlaceReg>();
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

// phase i's weights: every field group of the defaults scaled by a factor of its own per phase
hsddp_hkd_weights weights_of_phase(int i)
{
    hsddp_hkd_weights w;
    hsddp_default_weights(&w);
    const double f[3][6] = {{1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, {1.25, 0.8, 1.5, 0.75, 1.2, 0.5}, {0.7, 1.3, 0.9, 1.4, 0.85, 1.5}};
    for (int a = 0; a < 3; ++a) { w.q_eul[a] *= f[i][0]; w.q_pos[a] *= f[i][1]; w.q_omega[a] *= f[i][0]; w.q_v[a] *= f[i][1]; }
    w.q_qJ *= f[i][2];
    for (int j = 0; j < 24; ++j) w.qf_scale[j] *= f[i][3];
    w.r_grf *= f[i][4]; w.r_qJd *= f[i][5];
    for (int a = 0; a < 3; ++a) w.foot_w[a] = (w.foot_w[a] + 0.25 * a) * f[i][2];
    w.foot_term_cost *= f[i][4]; w.foot_term_grad *= f[i][3];
    return w;
}

// three trot phases of n0, 6, 6 knots whose cost objects differ (same: all on phase 0's weights)
std::vector<Built> problem(int n0, bool same, bool diag, int bad_phase = -1)
{
    std::vector<Built> p{hkd_phase(n0, A, B, 0.0, bad_phase == 0 ? 2 : diag), hkd_phase(6, B, A, 0.01 * n0, bad_phase == 1 ? 2 : diag),
                         hkd_phase(6, A, B, 0.01 * (n0 + 6), bad_phase == 2 ? 2 : diag)};
    for (int i = 0; i < 3; ++i) p[i].tc->weights = p[i].fr->weights = weights_of_phase(same ? 0 : i);
    return p;
}

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
    s.per_phase_weights = true;
    DVec<double> x0(24);
    for (int j = 0; j < 24; ++j) x0[j] = p[0].traj->Xbar[0][j];
    x0[3] += 0.01;
    s.set_initial_condition(x0);
}

bool same_row(const hsddp_hkd_weights &a, const hsddp_hkd_weights &b) { return !std::memcmp(&a, &b, sizeof a); }

// the diagonals the device forms from a row on contact c equal those of the phase's own weights
bool same_diagonals(const hsddp_hkd_weights &a, const hsddp_hkd_weights &b, const Arr &c)
{
    double qa[24], ra[24], fa[24], ga[12], qb[24], rb[24], fb[24], gb[12];
    hsddp_facade::device_diagonals(a, c.data(), qa, ra, fa, ga);
    hsddp_facade::device_diagonals(b, c.data(), qb, rb, fb, gb);
    return !std::memcmp(qa, qb, sizeof qa) && !std::memcmp(ra, rb, sizeof ra) && !std::memcmp(fa, fb, sizeof fa) &&
           !std::memcmp(ga, gb, sizeof ga) && a.foot_term_cost == b.foot_term_cost && a.foot_term_grad == b.foot_term_grad;
}

int host_checks()
{
    const Arr cs[3] = {A, B, A};
    {   // hkd:: terms: each phase's row is its objects' weights; phase 0's is the handle's
        MultiPhaseDDP<double> s;
        auto p = problem(6, false, false);
        install(s, p);
        const auto pr = s.describe();
        CHECK(pr.phase_weights.size() == 3 && pr.phase_weights_set.size() == 3);
        CHECK(same_row(pr.desc.weights, weights_of_phase(0)));
        for (int i = 0; i < 3; ++i) CHECK(same_row(pr.phase_weights[i], weights_of_phase(i)));
        CHECK(!pr.phase_weights_set[0] && pr.phase_weights_set[1] && pr.phase_weights_set[2]);
    }
    {   // diagonals alone: the quotient rule per phase reproduces every phase's diagonals bit for bit;
        // the fields a phase masks out are the handle-wide ones
        MultiPhaseDDP<double> s;
        auto p = problem(6, false, true);
        install(s, p);
        const auto pr = s.describe();
        CHECK(pr.phase_weights.size() == 3);
        for (int i = 0; i < 3; ++i) CHECK(same_diagonals(pr.phase_weights[i], weights_of_phase(i), cs[i]));
        CHECK(!pr.phase_weights_set[0] && pr.phase_weights_set[1] && pr.phase_weights_set[2]);
        CHECK(pr.phase_weights[1].qf_gain == pr.desc.weights.qf_gain && pr.phase_weights[1].foot_gain == pr.desc.weights.foot_gain);
    }
    for (int diag = 0; diag < 2; ++diag) {  // phases that agree: the handle's weights, no overrides
        MultiPhaseDDP<double> s;
        auto p = problem(6, true, diag != 0);
        install(s, p);
        const auto pr = s.describe();
        CHECK(pr.phase_weights.empty() && pr.phase_weights_set.empty());
        CHECK(same_diagonals(pr.desc.weights, weights_of_phase(0), A) && same_diagonals(pr.desc.weights, weights_of_phase(0), B));
    }
    {   // the phases move through the horizon: each keeps its row
        MultiPhaseDDP<double> s;
        auto p = problem(6, false, false);
        for (int tick = 1; tick < 3; ++tick) {
            tick_phases(p, tick);
            install(s, p);
            const auto pr = s.describe();
            CHECK(pr.desc.horizons[0] == 6 - tick && pr.desc.horizons[2] == 6 + tick);
            for (int i = 0; i < 3; ++i) CHECK(same_row(pr.phase_weights[i], weights_of_phase(i)));
        }
    }
    {   // qJ weight on a stance leg is no HKD pattern: still refused
        MultiPhaseDDP<double> s;
        auto p = problem(6, false, true, 1);
        install(s, p);
        bool refused = false;
        try {
            s.describe();
        } catch (const std::exception &e) {
            refused = std::strstr(e.what(), "not the HKD pattern") != nullptr;
        }
        CHECK(refused);
    }
    for (int diag = 0; diag < 2; ++diag) {  // without per_phase_weights (the default) differing phases are refused as before
        MultiPhaseDDP<double> s;
        auto p = problem(6, false, diag != 0);
        install(s, p);
        s.per_phase_weights = false;
        bool refused = false;
        try {
            s.describe();
        } catch (const std::exception &e) {
            refused = std::strstr(e.what(), "phase 1: tracking weights") != nullptr && std::strstr(e.what(), "per_phase_weights") != nullptr;
        }
        CHECK(refused);
    }
    std::printf("phase_weights_facade host ok\n");
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

// the C-ABI path on describe()'s arrays; rows: with hsddp_set_phase_weights
int abi_solve(const MultiPhaseDDP<double>::Problem &pr, const std::vector<double> &x0, const hsddp_options &o, bool rows,
              int tick, Solved &out)
{
    hsddp_handle h = nullptr;
    if (new_handle(pr, x0, o, h)) return 1;
    ABI(hsddp_upload_warm_start(h, pr.Xbar.data(), pr.Ubar.data(), pr.K.data()));
    ABI(hsddp_upload_constraint_params(h, pr.reb_delta.data(), pr.reb_eps.data(), pr.td_legs.data(), pr.al_sigma.data(),
                                       pr.al_lambda.data()));
    if (rows) ABI(hsddp_set_phase_weights(h, pr.phase_weights.data(), pr.phase_weights_set.data()));
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
    for (int diag = 0; diag < 2; ++diag) {
        MultiPhaseDDP<double> s;
        auto p = problem(6, false, diag != 0);
        for (int tick = 0; tick < 3; ++tick) {
            if (tick) tick_phases(p, tick);
            install(s, p);
            const auto pr = s.describe();
            CHECK(pr.phase_weights.size() == 3 && pr.phase_weights_set[1] && pr.phase_weights_set[2]);
            std::vector<double> x0(24);
            for (int j = 0; j < 24; ++j) x0[j] = p[0].traj->Xbar[0][j];
            x0[3] += 0.01;
            Solved a, n;
            if (abi_solve(pr, x0, o, true, tick, a) || abi_solve(pr, x0, o, false, tick, n)) return 1;
            s.solve(opt);  // (today's refusal came from here: one device handle holds one weight set)
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
            // (the rows are read: without hsddp_set_phase_weights the solve is another one)
            CHECK(!same(after.Ubar, n.Ubar));
            std::printf("%s tick %d: facade == C ABI with hsddp_set_phase_weights\n", diag ? "diagonals" : "hkd terms", tick);
        }
    }
    std::printf("phase_weights_facade device ok\n");
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
