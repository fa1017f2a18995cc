// restart_facade — HKDMPCSolver::restart (hkd-mpc_amd/facade/hkd_mpc.hpp) for tests/test_gpu_restart_tick.py:
// a batch with per-robot windows runs `ticks` updates on the robot states of <dir>/states.bin
// ([ticks][B] hsddp_robot_state); before update number `at` (1-based) the robots of <dir>/restart.txt
// ("robot window" per line) are restarted, with that tick's records as their states.  Every tick's
// commands go to <dir>/commands.bin ([ticks][B] hsddp_mpc_command), and the handle's state after
// every tick to <dir>/state.bin: S, Kc (int), Xbar [B][S][24], Ubar [B][Kc][24] (double), element
// info [B] (hsddp_element_info).
//
//   restart_facade <quad_reference.csv> <ddp_setting.info> <dir> <B> <ticks> <at> <plan_duration>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "hkd_mpc.hpp"

static hkd::hkd_data_lcmt message(const hsddp_robot_state &r, int t)
{
    hkd::hkd_data_lcmt m{};
    m.reset_mpc = false;
    m.MS = true;
    m.mpctime = 0.01 * t;
    for (int a = 0; a < 3; ++a) {
        m.p[a] = r.p[a]; m.vWorld[a] = r.vWorld[a]; m.rpy[a] = r.rpy[a]; m.omegaBody[a] = r.omegaBody[a];
    }
    for (int j = 0; j < 12; ++j) { m.qJ[j] = r.qJ[j]; m.foot_placements[j] = r.foot_placements[j]; }
    return m;
}

int main(int argc, char **argv)
{
    if (argc != 8) {
        std::fprintf(stderr, "usage: restart_facade ref.csv ddp.info dir B ticks at plan_duration\n");
        return 2;
    }
    const std::string dir = argv[3];
    const int B = std::atoi(argv[4]), ticks = std::atoi(argv[5]), at = std::atoi(argv[6]);
    try {
        std::vector<hsddp_robot_state> states((size_t)ticks * B);
        std::ifstream fs(dir + "/states.bin", std::ios::binary);
        if (!fs.read((char *)states.data(), (std::streamsize)(states.size() * sizeof(hsddp_robot_state)))) throw std::runtime_error("states.bin");
        std::vector<int> robots, windows;
        std::ifstream fr(dir + "/restart.txt");
        for (int b, w; fr >> b >> w;) { robots.push_back(b); windows.push_back(w); }
        hkd::HKDMPCSolver mpc(argv[1], B, argv[2]);
        mpc.mpc_config.plan_duration = (float)std::atof(argv[7]);
        mpc.mpc_config.per_robot_windows = true;
        mpc.initialize();
        std::FILE *out = std::fopen((dir + "/commands.bin").c_str(), "wb");
        if (!out) throw std::runtime_error("commands.bin");
        std::FILE *st_out = std::fopen((dir + "/state.bin").c_str(), "wb");
        if (!st_out) throw std::runtime_error("state.bin");
        mpc.set_publisher([&](const std::vector<hsddp_mpc_command> &c) { std::fwrite(c.data(), sizeof(hsddp_mpc_command), c.size(), out); });
        for (int t = 1; t <= ticks; ++t) {
            std::vector<hkd::hkd_data_lcmt> msgs(B);
            for (int b = 0; b < B; ++b) msgs[b] = message(states[(size_t)(t - 1) * B + b], t);
            if (t == at) {
                std::vector<hkd::hkd_data_lcmt> st;
                for (int b : robots) st.push_back(msgs[b]);
                mpc.restart(robots, windows, st);
            }
            mpc.mpcdata_lcm_handler(msgs);
            mpc.wait();
            int S = 0;
            if (hsddp_get_strides(mpc.h, nullptr, &S)) throw std::runtime_error(hsddp_last_error());
            std::vector<int> np(B), hzs((size_t)B * HSDDP_MAX_PHASES);
            if (hsddp_get_element_layouts(mpc.h, np.data(), hzs.data(), nullptr, nullptr)) throw std::runtime_error(hsddp_last_error());
            int Kc = 0;
            for (int i = 0; i < np[0]; ++i) Kc += hzs[i];
            std::vector<double> Xb((size_t)B * S * 24), Ub((size_t)B * Kc * 24);
            std::vector<hsddp_element_info> info = mpc.solver_info();
            if (hsddp_download_trajectory(mpc.h, Xb.data(), Ub.data(), nullptr)) throw std::runtime_error(hsddp_last_error());
            std::fwrite(&S, sizeof(int), 1, st_out);
            std::fwrite(&Kc, sizeof(int), 1, st_out);
            std::fwrite(Xb.data(), sizeof(double), Xb.size(), st_out);
            std::fwrite(Ub.data(), sizeof(double), Ub.size(), st_out);
            std::fwrite(info.data(), sizeof(hsddp_element_info), info.size(), st_out);
        }
        std::fclose(out);
        std::fclose(st_out);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "restart_facade: %s\n", e.what());
        return 1;
    }
    std::printf("restart_facade ok\n");
    return 0;
}
