// phases_check — the host phase bookkeeping (hkd-mpc_amd/csrc/hsddp_phases.cpp) on its own, without
// the product library or a GPU (tests/test_phases_host.py compares it with mpc_oracle.shift).
// stdin, one case per line: three comma-separated lists, `horizons reach_flags step_flags`.
// stdout, one line per case: `refused <code>`, or `ok` and the lists N, ss, reach, xs (state-slot
// labels), us (control-slot labels), src and add per phase, separated by blanks.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hkd-mpc_amd/csrc/hsddp_phases.h"

static std::vector<int> ints(const std::string &s)
{
    std::vector<int> v;
    std::stringstream ss(s);
    std::string w;
    while (std::getline(ss, w, ',')) v.push_back(std::stoi(w));
    return v;
}

static void put(const std::vector<int> &v)
{
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? "," : " ", v[i]);
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::stringstream ls(line);
        std::string a, b, c;
        if (!(ls >> a >> b >> c)) continue;
        const std::vector<int> hz = ints(a), reach = ints(b), flags = ints(c);
        if (reach.size() != hz.size()) { std::fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        hsddp::Layout L, Ln;
        std::string why;
        int rc = hsddp::build_layout((int)hz.size(), hz.data(), nullptr, L, why);
        if (!rc) {
            hsddp::PhaseStepper st(L, reach.data());
            for (size_t j = 0; j < flags.size() && !rc; ++j)
                if (!(rc = st.drop_front("shift", why))) rc = st.extend_back(flags[j], "shift", why);
            if (!rc) rc = st.finish(Ln, why);
            if (!rc) {
                std::vector<int> N, ss, re, xs, us, src, add;
                for (const hsddp::ShiftPhase &f : st.ph) {
                    N.push_back(f.N); ss.push_back(f.ss); re.push_back(f.reach);
                    xs.insert(xs.end(), f.xs.begin(), f.xs.end());
                    us.insert(us.end(), f.us.begin(), f.us.end());
                    src.push_back(f.src); add.push_back(f.add);
                }
                // the layout finish() returns is the phases' own
                if (Ln.P != (int)N.size() || Ln.S != (int)xs.size()) { std::fprintf(stderr, "layout mismatch: %s\n", line.c_str()); return 3; }
                std::printf("ok");
                for (const std::vector<int> *v : {&N, &ss, &re, &xs, &us, &src, &add}) put(*v);
                std::printf("\n");
                continue;
            }
        }
        std::printf("refused %d\n", rc);
    }
    return 0;
}
