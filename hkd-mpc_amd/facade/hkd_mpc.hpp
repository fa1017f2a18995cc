// hkd_mpc.hpp — HKDMPCSolver (HKDMPC/HKDMPC.h:22-100, HKDMPC.cpp:18-298) over the C-ABI, for a
// batch of B robots on one GPU, with the reference's member names and call sequence:
//
//   HKDMPCSolver(reference_file)      loads the quad_reference.csv     (HKDMPC.h:26-31)
//   initialize()                      HKDProblem::initialization + first solve (HKDMPC.cpp:20-94)
//   mpcdata_lcm_handler(msgs)         copies the robot states, starts update() on a worker
//                                     thread (HKDMPC.cpp:166-200)
//   update()                          HKDProblem::update + re-solve with max_AL_iter = 2,
//                                     max_DDP_iter = 1 + update_foot_placement + publish_mpc_cmd
//                                     (HKDMPC.cpp:96-165, 207-298)
//   simulate_policy(...)              the solved policy simulated from given states
//                                     (hsddp_simulate_policy)
//   restart(robots, windows, states)  the named robots start again as new problems in the next
//                                     update(): HKDMPCSolver::initialize for them (HKDMPC.cpp:20-94)
//                                     beside ::update for the rest (hsddp_restart_elements,
//                                     hsddp_set_element_budgets; mpc_config.per_robot_windows)
//   update_closed_loop()              update() with the plant on the device: the next initial state
//                                     is the policy's own simulation of the steps between two updates
//                                     (closed_loop = true makes the message handler run it)
//
// Device-side: the phase bookkeeping, warm-start shift, per-knot references, the initial state from
// the measured robot states, solve and command extraction (hsddp_advance,
// hsddp_update_problem_measured, hsddp_solve, hsddp_extract_commands_measured); per tick only the B
// robot states (144 bytes each) go up and the B commands come back.  LCM is not available on this platform: a message
// is the hkd_data_lcmt struct below and publishing calls a user callback with the
// hkd_command_lcmt records (hsddp_mpc_command).  The worker serialises updates as mpc_mutex does
// in the reference (a new request waits for the running update); wait() joins it.
#ifndef HKD_MPC_HPP
#define HKD_MPC_HPP

#include <chrono>
#include <cmath>
#include <exception>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hsddp.h"

namespace hkd {

// hkd_data_lcmt (lcmtypes/hkd_data_lcmt.lcm:1-12), one robot
struct hkd_data_lcmt {
    bool reset_mpc;
    bool MS;
    double mpctime;
    int contact[4];
    float p[3], vWorld[3], rpy[3], omegaBody[3], qJ[12], foot_placements[12];
};

// HKDProblem's configuration (HKDMPC.cpp:26-29)
struct MPCConfig {
    float plan_duration = 0.6f;
    int nsteps_between_mpc = 1;
    float timeStep = 0.01f;
    // every robot with its own reference window and phase layout (desc.ref_per_element): robots can
    // then be restarted one by one (restart()); off: the batch shares one window, as one robot's
    bool per_robot_windows = false;
};

class HKDMPCSolver {
public:
    using Publisher = std::function<void(const std::vector<hsddp_mpc_command> &)>;

    // reference_file: quad_reference.csv; batch: robots solved together; settings: ddp_setting.info
    HKDMPCSolver(const std::string &reference_file, int batch, const std::string &settings, int device = 0)
        : B(batch), dev(device), settings_file(settings)
    {
        const int n = hsddp_load_quad_reference(reference_file.c_str(), 0, &dt_ref, nullptr, 0);
        if (n <= 0) throw std::runtime_error(std::string("reference: ") + hsddp_last_error());
        quad_reference.resize(n);
        hsddp_load_quad_reference(reference_file.c_str(), 0, &dt_ref, quad_reference.data(), n);
        hkd_data.resize(B);
        solve_time = 0;
    }
    ~HKDMPCSolver()
    {
        if (worker.joinable()) worker.join();
        if (h) hsddp_destroy(h);
    }
    HKDMPCSolver(const HKDMPCSolver &) = delete;
    HKDMPCSolver &operator=(const HKDMPCSolver &) = delete;

    void set_publisher(Publisher p) { publish = std::move(p); }

    // HKDMPCSolver::initialize (HKDMPC.cpp:20-94): options from the INFO file, the phase plan of
    // the window at the reference's start (QuadReference::initialize), references on the device,
    // the nominal initial state, one full solve
    void initialize()
    {
        std::lock_guard<std::mutex> lk(mpc_mutex);
        hsddp_default_options(&ddp_options);
        chk(hsddp_load_settings(settings_file.c_str(), &ddp_options));
        const int n_win = (int)std::lround(mpc_config.plan_duration / dt_ref) + 2;
        if ((int)quad_reference.size() < n_win) throw std::runtime_error("reference shorter than the plan window");
        dt_mpc = mpc_config.timeStep * mpc_config.nsteps_between_mpc;
        hsddp_phase_plan plan;
        chk(hsddp_plan_phases(quad_reference.data(), n_win, dt_ref, mpc_config.plan_duration, mpc_config.timeStep,
                              dt_mpc, &plan));
        if (h) { hsddp_destroy(h); h = nullptr; }
        hsddp_problem_desc desc{};
        desc.device = dev;
        desc.batch = B;
        desc.n_phases = plan.n_phases;
        for (int i = 0; i < plan.n_phases; ++i) desc.horizons[i] = plan.horizons[i];
        desc.dt = mpc_config.timeStep;
        desc.ref_per_element = mpc_config.per_robot_windows ? 1 : 0;
        hsddp_default_weights(&desc.weights);
        hsddp_default_constraint_params(&desc.cparams);
        chk(hsddp_create(&desc, &h));
        chk(hsddp_set_options(h, &ddp_options));
        chk(hsddp_set_reference_table(h, quad_reference.data(), (int)quad_reference.size(), dt_ref));
        const std::vector<int> ws(mpc_config.per_robot_windows ? B : 1, 0);
        chk(hsddp_build_references(h, ws.data(), n_win, nullptr, mpc_config.timeStep));
        P = plan.n_phases;
        std::vector<int> contacts((size_t)B * (P + 1) * 4);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i <= P; ++i)
                for (int l = 0; l < 4; ++l) contacts[((size_t)b * (P + 1) + i) * 4 + l] = plan.contacts[i][l];
        // xinit = [body, qdummy]: body = (eul 0, pos (0, 0, 0.2486), 0, 0), qJ = (0, -0.8, 1.6) x 4
        // (HKDMPC.cpp:44-55)
        std::vector<double> x0((size_t)B * 24, 0.0);
        for (int b = 0; b < B; ++b) {
            double *x = &x0[(size_t)b * 24];
            x[5] = 0.2486;
            for (int j = 0; j < 12; ++j) x[12 + j] = j % 3 == 0 ? 0.0 : (j % 3 == 1 ? -0.8 : 1.6);
        }
        compute_hkd_state(x0, contacts, P);
        chk(hsddp_upload_problem(h, contacts.data(), x0.data(), nullptr, nullptr, nullptr));
        hsddp_stats st;
        chk(hsddp_solve(h, &st));
        mpc_time = 0;
        mpc_time_prev = 0;
        mpc_iter = 0;
        mpc_time0.assign(B, 0.0);
        restarted.assign(B, 0);
        pending_robots.clear();
    }

    // The named robots start again in the next update(), each as a new problem at table sample
    // window_starts[j] with the measured state states[j] (which replaces that robot's message for
    // the tick).  The tick's order is advance -> restart -> x0 -> solve: advancing a robot that is
    // then restarted is harmless, because the restart overwrites everything the advance touched
    // for it.  The restarted robots solve with the options' max_AL_iter / max_DDP_iter, as
    // initialize() does, the others with update()'s pair (quirk A17), in the same solve; a restarted
    // robot's mpc_time starts from 0 again, as after initialize().
    void restart(const std::vector<int> &robots, const std::vector<int> &window_starts,
                 const std::vector<hkd_data_lcmt> &states)
    {
        if (robots.size() != window_starts.size() || robots.size() != states.size())
            throw std::runtime_error("restart: one window start and one state per robot");
        for (int b : robots)
            if (b < 0 || b >= B) throw std::runtime_error("restart: no such robot");
        wait();
        std::lock_guard<std::mutex> lk(mpc_mutex);
        pending_robots = robots;
        pending_windows = window_starts;
        pending_states = states;
    }

    // Per-robot terrain (hsddp_set_terrain): the robot's friction coefficient and touchdown ground
    // height on every phase of its horizon, from the next solve on.  The rows move with the robot's
    // phases (a phase entering the horizon takes the row of the one before it), so one call lasts
    // until the next; restart() and initialize() return a robot to the settings' pair.  Within a
    // tick the order is advance -> (restart) -> set_terrain -> x0 -> solve: call between ticks.
    void set_terrain(int robot, double mu, double ground)
    {
        if (robot < 0 || robot >= B) throw std::runtime_error("set_terrain: no such robot");
        wait();
        std::lock_guard<std::mutex> lk(mpc_mutex);
        int Ps = 0;
        chk(hsddp_get_strides(h, &Ps, nullptr));
        std::vector<double> m((size_t)B * Ps), g((size_t)B * Ps);
        chk(hsddp_get_terrain(h, m.data(), g.data()));
        for (int i = 0; i < Ps; ++i) {
            m[(size_t)robot * Ps + i] = mu;
            g[(size_t)robot * Ps + i] = ground;
        }
        chk(hsddp_set_terrain(h, m.data(), g.data()));
    }

    // Per-robot cost weights (hsddp_set_element_weights): the robot's HKD weights from the next solve
    // on, where the settings give one set for the batch.  The row belongs to the robot: it stays
    // through every tick and through restart().  Call between ticks.
    void set_weights(int robot, const hsddp_hkd_weights &w)
    {
        if (robot < 0 || robot >= B) throw std::runtime_error("set_weights: no such robot");
        wait();
        std::lock_guard<std::mutex> lk(mpc_mutex);
        std::vector<hsddp_hkd_weights> rows((size_t)B, w);
        std::vector<int> mask((size_t)B, 0);
        mask[(size_t)robot] = 1;
        chk(hsddp_set_element_weights(h, rows.data(), mask.data()));
    }

    // Per-phase cost weights (hsddp_set_phase_weights): phase `phase` of the robot's current horizon
    // takes w as its override from the next solve on, as a cost object of that phase would hold it.
    // The override moves with its phase through the ticks and leaves with it; a phase the horizon
    // appends has none and reads the robot's row (set_weights) or the settings'; restart() drops the
    // robot's overrides.  Call between ticks.
    void set_phase_weights(int robot, int phase, const hsddp_hkd_weights &w)
    {
        if (robot < 0 || robot >= B) throw std::runtime_error("set_phase_weights: no such robot");
        wait();
        std::lock_guard<std::mutex> lk(mpc_mutex);
        int P = 0, S = 0;
        chk(hsddp_get_strides(h, &P, &S));
        std::vector<int> np((size_t)B, P);
        chk(hsddp_get_element_layouts(h, np.data(), nullptr, nullptr, nullptr));
        if (phase < 0 || phase >= np[(size_t)robot]) throw std::runtime_error("set_phase_weights: the robot has no such phase");
        // the C ABI takes [B][P] arrays and reads only the masked entry: buffers kept from call to
        // call (grown at a new stride), one row written and one flag set and cleared again
        const size_t n = (size_t)B * P, q = (size_t)robot * P + phase;
        if (pw_rows.size() < n) pw_rows.resize(n);
        if (pw_mask.size() < n) pw_mask.resize(n, 0);
        pw_rows[q] = w;
        pw_mask[q] = 1;
        const int rc = hsddp_set_phase_weights(h, pw_rows.data(), pw_mask.data());
        pw_mask[q] = 0;
        chk(rc);
    }

    // HKDMPCSolver::mpcdata_lcm_handler (HKDMPC.cpp:166-200): msgs[B]
    void mpcdata_lcm_handler(const std::vector<hkd_data_lcmt> &msgs)
    {
        if ((int)msgs.size() != B) throw std::runtime_error("one message per robot");
        wait();  // mpc_mutex: the previous update finishes first
        if (msgs[0].reset_mpc) {
            ddp_options.MS = msgs[0].MS;
            initialize();
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mpc_mutex);
            hkd_data = msgs;
            mpc_time_prev = mpc_time;
            mpc_time = msgs[0].mpctime;
        }
        worker = std::thread([this] {
            try {
                if (closed_loop) update_closed_loop();
                else update();
            } catch (...) {
                worker_error = std::current_exception();
            }
        });
    }

    // joins the running update; rethrows its failure
    void wait()
    {
        if (worker.joinable()) worker.join();
        if (worker_error) {
            std::exception_ptr e = worker_error;
            worker_error = nullptr;
            std::rethrow_exception(e);
        }
    }

    // HKDMPCSolver::update (HKDMPC.cpp:96-165).  The messages' state fields go up as they are
    // (hsddp_robot_state has hkd_data_lcmt's fields in its order); xinit is formed on the device
    // from each robot's new first-phase contact, and the extraction reads the foot placements and
    // the phases' contact durations from the handle: no host model arithmetic, no round trip.
    void update()
    {
        std::lock_guard<std::mutex> lk(mpc_mutex);
        hsddp_options o = ddp_options;
        o.max_AL_iter = 2;  // quirk A17
        o.max_DDP_iter = 1;
        chk(hsddp_set_options(h, &o));
        mpc_iter++;
        for (size_t j = 0; j < pending_robots.size(); ++j) hkd_data[pending_robots[j]] = pending_states[j];
        robot_states.resize(B);
        for (int b = 0; b < B; ++b) {
            const hkd_data_lcmt &m = hkd_data[b];
            hsddp_robot_state &r = robot_states[b];
            for (int a = 0; a < 3; ++a) {
                r.p[a] = m.p[a];
                r.vWorld[a] = m.vWorld[a];
                r.rpy[a] = m.rpy[a];
                r.omegaBody[a] = m.omegaBody[a];
            }
            for (int j = 0; j < 12; ++j) {
                r.qJ[j] = m.qJ[j];
                r.foot_placements[j] = m.foot_placements[j];
            }
        }
        // opt_problem.update(): layout, warm start, references; then xinit = [eul, pos, omega, vel,
        // qdummy] from the robot states (HKDMPC.cpp:118-134) with the contacts the advance derived
        std::vector<int> flags(mpc_config.nsteps_between_mpc);
        chk(hsddp_advance(h, mpc_config.nsteps_between_mpc, mpc_config.plan_duration, dt_mpc, nullptr, flags.data()));
        if (!pending_robots.empty()) {  // (after the advance: the restart overwrites what it did to these robots)
            std::vector<int> mask(B, 0), ws(B, 0), al(B, o.max_AL_iter), ddp(B, o.max_DDP_iter);
            for (size_t j = 0; j < pending_robots.size(); ++j) {
                const int b = pending_robots[j];
                mask[b] = 1;
                ws[b] = pending_windows[j];
                al[b] = ddp_options.max_AL_iter;   // HKDMPCSolver::initialize's budget
                ddp[b] = ddp_options.max_DDP_iter;
                mpc_time0[b] = mpc_time;
                restarted[b] = 1;
            }
            chk(hsddp_restart_elements(h, mask.data(), ws.data(), mpc_config.plan_duration, dt_mpc, nullptr));
            chk(hsddp_set_element_budgets(h, al.data(), ddp.data()));
        } else {
            chk(hsddp_set_element_budgets(h, nullptr, nullptr));
        }
        pending_robots.clear();
        chk(hsddp_update_problem_measured(h, nullptr, robot_states.data(), 0, nullptr, nullptr, nullptr));
        const auto t0 = std::chrono::high_resolution_clock::now();
        hsddp_stats st;
        chk(hsddp_solve(h, &st));
        const auto t1 = std::chrono::high_resolution_clock::now();
        solve_time = (float)std::chrono::duration<double, std::milli>(t1 - t0).count();
        // update_foot_placement + publish_mpc_cmd (HKDMPC.cpp:207-298)
        commands.resize(B);
        chk(hsddp_extract_commands_measured(h, mpc_config.nsteps_between_mpc, mpc_time, dt_mpc, nullptr, 0, solve_time,
                                            commands.data(), 0));
        // a robot restarted at mpc_time t0 counts its own time from there (rounded twice, as the
        // extraction rounds mpc_time + k dt_mpc)
        for (int b = 0; b < B; ++b) {
            if (!restarted[b]) continue;
            const double tb = mpc_time - mpc_time0[b];
            for (int k = 0; k < commands[b].N_mpcsteps; ++k) {
                // the product is rounded before the sum, as the device forms it: the volatile keeps
                // the compiler from contracting the two into one fused multiply-add
                volatile double step = (double)k * (double)dt_mpc;
                commands[b].mpc_times[k] = tb + step;
            }
        }
        if (publish) publish(commands);
        // P and the durations member, for callers that read them: host copies of what the handle
        // holds, after the commands have left (P: the largest robot's with per-robot layouts)
        std::vector<int> nph(B);
        chk(hsddp_get_element_layouts(h, nph.data(), nullptr, nullptr, nullptr));
        P = 0;
        for (int v : nph) P = v > P ? v : P;
        durations.assign((size_t)B * P * 4, 0.0);
        chk(hsddp_get_phase_info(h, nullptr, durations.data()));
    }

    // hsddp_simulate_policy for the batch: n_samples states per robot, n_steps knots each (x_init
    // [B][n_samples][24] or null: the robots' current x0; outputs may be null)
    void simulate_policy(int n_samples, int n_steps, const double *x_init, double *x_end, hsddp_sim_sample *summary,
                         double *X = nullptr, double *U = nullptr)
    {
        chk(hsddp_simulate_policy(h, n_samples, n_steps, x_init, x_end, summary, X, U));
    }

    // update() with the plant in the loop: the policy of the last solve is simulated for the
    // nsteps_between_mpc steps from the handle's x0 (one sample per robot), the problem advances
    // with its inputs pending, and the simulation's end states become the new initial states on
    // the device (hsddp_update_problem_simulated: no FK round trip, no x0 upload).  The messages
    // still give mpctime and the current foot placements.
    void update_closed_loop()
    {
        std::lock_guard<std::mutex> lk(mpc_mutex);
        hsddp_options o = ddp_options;
        o.max_AL_iter = 2;  // quirk A17
        o.max_DDP_iter = 1;
        chk(hsddp_set_options(h, &o));
        mpc_iter++;
        const int n = mpc_config.nsteps_between_mpc;
        plant.resize(B);
        chk(hsddp_simulate_policy(h, 1, n, nullptr, nullptr, plant.data(), nullptr, nullptr));
        std::vector<int> flags(n);
        chk(hsddp_advance(h, n, mpc_config.plan_duration, dt_mpc, nullptr, flags.data()));
        int hz[HSDDP_MAX_PHASES];
        chk(hsddp_get_layout(h, &P, hz, nullptr, nullptr));
        durations.assign((size_t)B * P * 4, 0.0);
        chk(hsddp_get_phase_info(h, nullptr, durations.data()));
        chk(hsddp_update_problem_simulated(h, 0));
        const auto t0 = std::chrono::high_resolution_clock::now();
        hsddp_stats st;
        chk(hsddp_solve(h, &st));
        const auto t1 = std::chrono::high_resolution_clock::now();
        solve_time = (float)std::chrono::duration<double, std::milli>(t1 - t0).count();
        std::vector<float> pf((size_t)B * 12);
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < 12; ++j) pf[(size_t)b * 12 + j] = hkd_data[b].foot_placements[j];
        commands.resize(B);
        chk(hsddp_extract_commands(h, n, mpc_time, dt_mpc, durations.data(), 1, pf.data(), 1, solve_time,
                                   commands.data()));
        if (publish) publish(commands);
    }

    // per-element results of the last solve
    std::vector<hsddp_element_info> solver_info() const
    {
        std::vector<hsddp_element_info> info(B);
        chk(hsddp_download_element_info(h, info.data()));
        return info;
    }

    int B, dev;
    std::string settings_file;
    MPCConfig mpc_config;
    hsddp_options ddp_options{};
    std::vector<hsddp_quad_state> quad_reference;
    float dt_ref = 0, dt_mpc = 0.01f;
    std::vector<hkd_data_lcmt> hkd_data;
    std::vector<hsddp_mpc_command> commands;
    std::vector<double> durations;                 // the phases' contact durations after the last update
    std::vector<hsddp_robot_state> robot_states;   // the messages' state fields as update() sent them
    bool closed_loop = false;              // the message handler runs update_closed_loop()
    std::vector<hsddp_sim_sample> plant;   // the plant's outcome per robot in the last closed-loop update
    double mpc_time = 0, mpc_time_prev = 0;
    std::vector<double> mpc_time0;  // per robot: the mpc_time of its last restart
    std::vector<char> restarted;    // per robot: restarted since initialize() (mpc_time0 holds a time)
    float solve_time;
    int mpc_iter = 0, P = 0;
    hsddp_handle h = nullptr;

private:
    static void chk(int rc)
    {
        if (rc != HSDDP_OK) throw std::runtime_error(std::string("hsddp: ") + hsddp_last_error());
    }

    // compute_hkd_state (HKD-TrajOpt/HKDModel.h:65-96) for every robot: the qdummy of a stance leg
    // of the first phase is its foot position, computed on the device (hsddp_hkd_foot_position);
    // of a swing leg the joint angles already in x
    void compute_hkd_state(std::vector<double> &x0, const std::vector<int> &contacts, int n_phases)
    {
        const size_t n = (size_t)B * 4;
        std::vector<int> leg(n);
        std::vector<double> xs(n * 24), pfo(n * 3);
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < 4; ++l) {
                leg[(size_t)b * 4 + l] = l;
                std::copy(&x0[(size_t)b * 24], &x0[(size_t)b * 24] + 24, &xs[((size_t)b * 4 + l) * 24]);
            }
        void *dx = hsddp_device_alloc(xs.size() * 8, dev), *dl = hsddp_device_alloc(n * 4, dev),
             *dp = hsddp_device_alloc(pfo.size() * 8, dev);
        int rc = (!dx || !dl || !dp) ? HSDDP_ERR_ALLOC : HSDDP_OK;
        if (!rc) rc = hsddp_memcpy_h2d(dx, xs.data(), xs.size() * 8);
        if (!rc) rc = hsddp_memcpy_h2d(dl, leg.data(), n * 4);
        if (!rc) rc = hsddp_hkd_foot_position((const double *)dx, (const int *)dl, (double *)dp, (int)n, nullptr);
        if (!rc) rc = hsddp_device_synchronize(dev);
        if (!rc) rc = hsddp_memcpy_d2h(pfo.data(), dp, pfo.size() * 8);
        hsddp_device_free(dx); hsddp_device_free(dl); hsddp_device_free(dp);
        chk(rc);
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < 4; ++l)
                if (contacts[((size_t)b * (n_phases + 1)) * 4 + l])
                    for (int a = 0; a < 3; ++a) x0[(size_t)b * 24 + 12 + 3 * l + a] = pfo[((size_t)b * 4 + l) * 3 + a];
    }

    std::vector<int> pending_robots, pending_windows;  // restart(): applied by the next update()
    std::vector<hkd_data_lcmt> pending_states;
    std::mutex mpc_mutex;
    std::vector<hsddp_hkd_weights> pw_rows;  // set_phase_weights' [B][P] arguments (mask all zero between calls)
    std::vector<int> pw_mask;
    std::thread worker;
    std::exception_ptr worker_error;
    Publisher publish;
};

}  // namespace hkd

#endif
