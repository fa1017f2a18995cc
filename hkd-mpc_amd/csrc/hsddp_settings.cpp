// hsddp_settings.cpp — the defaults of the option, weight and constraint-parameter blocks of
// include/hsddp.h and the INFO-file loaders (loadHSDDPSetting, HSDDP_CompoundTypes.h:62-87;
// loadConstrintParameters, HKDProblem.h:70-90).  Host only.
#include <cctype>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "hsddp_handle.h"

using hsddp::fail;

extern "C" void hsddp_default_options(hsddp_options *o)
{
    // HSDDP_OPTION in-class defaults (HSDDP_CompoundTypes.h:20-45)
    o->alpha = 0.1; o->gamma = 0.1; o->update_penalty = 8; o->update_relax = 0.1;
    o->update_regularization = 2; o->update_ReB = 7;
    o->max_DDP_iter = 3; o->max_AL_iter = 2; o->max_DDP_iter_runtime = 1; o->max_AL_iter_runtime = 2;
    o->cost_thresh = 1e-3; o->tconstr_thresh = 1e-3; o->pconstr_thresh = 1e-3; o->dynamics_feas_thresh = 1e-3;
    o->merit_rho = 1e4; o->merit_scale = 0.2; o->merit_offset = 10;
    o->AL_active = 1; o->ReB_active = 1; o->smooth_active = 0; o->MS = 1; o->nsteps_per_node = 1;
    o->no_early_exit = 0;
}

extern "C" void hsddp_default_weights(hsddp_hkd_weights *w)
{
    const double qe[3] = {1, 4, 5}, qp[3] = {1, 1, 30}, qo[3] = {.2, .2, .2}, qv[3] = {4, 1, .5};
    const double sc[24] = {1, 1, 2, 1, 1, 20, .3, .3, .3, 1, 3, 1, .01, .01, .01, .01, .01, .01, .01, .01, .01, .01, .01, .01};
    for (int i = 0; i < 3; ++i) { w->q_eul[i] = qe[i]; w->q_pos[i] = qp[i]; w->q_omega[i] = qo[i]; w->q_v[i] = qv[i]; }
    w->q_qJ = 0.2;
    for (int i = 0; i < 24; ++i) w->qf_scale[i] = sc[i];
    w->qf_gain = 20; w->r_grf = 0.2; w->r_qJd = 0.1;
    w->foot_w[0] = 3; w->foot_w[1] = 1; w->foot_w[2] = 0; w->foot_gain = 20;
    w->foot_term_cost = 10; w->foot_term_grad = 20;
}

extern "C" void hsddp_default_constraint_params(hsddp_constraint_params *cp)
{
    // settings/constraint_params.info values; mu = 0.7 (HKDConstraints.h:17); ground height 0
    cp->grf_delta = 0.1; cp->grf_delta_min = 0.1; cp->grf_eps = 0.1;
    cp->swing_delta = 1.0; cp->swing_delta_min = 0.5; cp->swing_eps = 0.01;
    cp->td_sigma = 50; cp->td_sigma_max = 1e4; cp->td_lambda = 0;
    cp->mu_fric = 0.7; cp->ground_height = 0.0;
}

// Minimal Boost.PropertyTree INFO reader: `key value` pairs, `key { ... }` children, ';' comments,
// optional double quotes.  Produces dotted paths ("ddp.alpha").
static int parse_info(const char *path, std::map<std::string, std::string> &out)
{
    std::ifstream f(path);
    if (!f) return fail(HSDDP_ERR_IO, std::string("cannot open ") + path);
    std::vector<std::string> stack;
    std::string line, last_key;
    while (std::getline(f, line)) {
        // strip comment (outside quotes)
        bool q = false;
        for (size_t i = 0; i < line.size(); ++i) {
            if (line[i] == '"') q = !q;
            if (line[i] == ';' && !q) { line.resize(i); break; }
        }
        std::vector<std::string> tok;
        std::string cur;
        q = false;
        for (char ch : line) {
            if (ch == '"') { q = !q; continue; }
            if (!q && (std::isspace((unsigned char)ch) || ch == '{' || ch == '}')) {
                if (!cur.empty()) { tok.push_back(cur); cur.clear(); }
                if (ch == '{' || ch == '}') tok.push_back(std::string(1, ch));
                continue;
            }
            cur += ch;
        }
        if (!cur.empty()) tok.push_back(cur);
        size_t i = 0;
        while (i < tok.size()) {
            if (tok[i] == "{") {
                stack.push_back(last_key);
                ++i;
                continue;
            }
            if (tok[i] == "}") {
                if (stack.empty()) return fail(HSDDP_ERR_IO, std::string("unbalanced '}' in ") + path);
                stack.pop_back();
                ++i;
                continue;
            }
            std::string key = tok[i++];
            std::string val;
            if (i < tok.size() && tok[i] != "{" && tok[i] != "}") val = tok[i++];
            std::string full;
            for (auto &s : stack) full += s + ".";
            full += key;
            out[full] = val;
            last_key = key;
        }
    }
    if (!stack.empty()) return fail(HSDDP_ERR_IO, std::string("unbalanced '{' in ") + path);
    return HSDDP_OK;
}

static int get_num(const std::map<std::string, std::string> &m, const std::string &k, double &v)
{
    auto it = m.find(k);
    if (it == m.end()) return fail(HSDDP_ERR_IO, "No such node (" + k + ")"); // ptree_bad_path
    char *end = nullptr;
    v = std::strtod(it->second.c_str(), &end);
    if (end == it->second.c_str() || *end) return fail(HSDDP_ERR_IO, "conversion of data failed (" + k + ")");
    return HSDDP_OK;
}
static int get_int(const std::map<std::string, std::string> &m, const std::string &k, int &v)
{
    auto it = m.find(k);
    if (it == m.end()) return fail(HSDDP_ERR_IO, "No such node (" + k + ")");
    char *end = nullptr;
    long x = std::strtol(it->second.c_str(), &end, 10);
    if (end == it->second.c_str() || *end) return fail(HSDDP_ERR_IO, "conversion of data failed (" + k + ")");
    v = (int)x;
    return HSDDP_OK;
}
static int get_bool(const std::map<std::string, std::string> &m, const std::string &k, int &v)
{
    auto it = m.find(k);
    if (it == m.end()) return fail(HSDDP_ERR_IO, "No such node (" + k + ")");
    const std::string &s = it->second;
    if (s == "true" || s == "1") v = 1;
    else if (s == "false" || s == "0") v = 0;
    else return fail(HSDDP_ERR_IO, "conversion of data failed (" + k + ")");
    return HSDDP_OK;
}

extern "C" int hsddp_load_settings(const char *path, hsddp_options *o)
{
    if (!path || !o) return fail(HSDDP_ERR_ARG, "null argument");
    std::map<std::string, std::string> m;
    int rc = parse_info(path, m);
    if (rc) return rc;
    hsddp_options t = *o;
    // exactly the keys loadHSDDPSetting reads (HSDDP_CompoundTypes.h:70-86); update_regularization and
    // smooth_active are not read, so they keep the caller's values (quirk A1).
#define N_(k) if ((rc = get_num(m, "ddp." #k, t.k))) return rc
#define I_(k) if ((rc = get_int(m, "ddp." #k, t.k))) return rc
#define B_(k) if ((rc = get_bool(m, "ddp." #k, t.k))) return rc
    N_(alpha); N_(gamma); N_(update_penalty); N_(update_relax); N_(update_ReB);
    I_(max_DDP_iter); I_(max_AL_iter); I_(max_DDP_iter_runtime); I_(max_AL_iter_runtime);
    N_(cost_thresh); N_(tconstr_thresh); N_(pconstr_thresh); N_(dynamics_feas_thresh);
    N_(merit_rho); N_(merit_scale); N_(merit_offset);
    B_(AL_active); B_(ReB_active); B_(MS); I_(nsteps_per_node);
#undef N_
#undef I_
#undef B_
    *o = t;
    return HSDDP_OK;
}

extern "C" int hsddp_load_constraint_params(const char *path, hsddp_constraint_params *cp)
{
    if (!path || !cp) return fail(HSDDP_ERR_ARG, "null argument");
    std::map<std::string, std::string> m;
    int rc = parse_info(path, m);
    if (rc) return rc;
    hsddp_constraint_params t = *cp;
    if ((rc = get_num(m, "GRF_ReB.delta", t.grf_delta)) || (rc = get_num(m, "GRF_ReB.delta_min", t.grf_delta_min)) ||
        (rc = get_num(m, "GRF_ReB.eps", t.grf_eps)) || (rc = get_num(m, "Swing_ReB.delta", t.swing_delta)) ||
        (rc = get_num(m, "Swing_ReB.delta_min", t.swing_delta_min)) || (rc = get_num(m, "Swing_ReB.eps", t.swing_eps)) ||
        (rc = get_num(m, "TD_AL.sigma", t.td_sigma)) || (rc = get_num(m, "TD_AL.lambda", t.td_lambda)) ||
        (rc = get_num(m, "TD_AL.sigma_max", t.td_sigma_max)))
        return rc;
    *cp = t;
    return HSDDP_OK;
}

