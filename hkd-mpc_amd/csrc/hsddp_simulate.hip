// hsddp_simulate.hip — the solved feedback policy applied to caller-given states (hsddp_simulate_policy).
//
// The simulated branch of SinglePhase::hybrid_rollout at eps = 0 (SinglePhase.cpp:196-222):
// U = Ubar + K (X - Xbar), X+ = hkinodyn(X, U), with MultiPhaseDDP::hybrid_rollout's reset map
// between phases (MultiPhaseDDP.cpp:73-81) and the 1e6 bound on the simulated state
// (SinglePhase.cpp:205-208), for M samples of every element from states the caller names.  Reads
// the handle's nominal trajectory, gains, references and contacts; writes only SimArgs' buffers.
#include "hsddp_simulate.h"

#include "hsddp_device.h"
#include "hsddp_dispatch.h"

namespace hsddp {

// One 64-lane wave per (element, chunk of 64 samples), lane = sample.  Xbar, Ubar, the gain rows,
// the reference rows, the contacts and the phase walk are the element's, the same for every lane:
// a wave reads each once.  A lane keeps its state in registers (every state and control index
// below is a compile-time one).  Lanes past M and lanes whose sample has broken the bound stop
// (live = false) while their neighbours go on; the knot loop ends when none is left.
//
// The element's rows of a knot (PK doubles below) come through LDS: at the top of knot kc the lanes
// issue one coalesced load each per 64 entries of knot kc + 1's rows, which stay in flight while
// knot kc is computed, and store them to the block's stage before knot kc + 1 starts; the knot
// reads them from there at compile-time offsets (every lane the same address: a broadcast).  With
// one wave per SIMD (413 registers) nothing else would hide the HBM latency of a knot's dependent
// loads: reading the rows directly took twice as long.  The fp32 gains are widened
// on the way in, so the knot has one arithmetic path.
constexpr int PK_XB = 0, PK_UB = 24, PK_K = 48, PK_XR = PK_K + KCW, PK_UR = PK_XR + 24, PK_PF = PK_UR + 24,
              PK_C = PK_PF + 12, PK = PK_C + 4;  // (PK_C: the contact rows c_i, c_{i+1}, 8 ints)
constexpr int PK_T = (PK + 63) / 64;
static_assert(PK == 400 && PK_T == 7, "stage layout");

// where knot kc of element b lives: phase i, knot k of the phase, state slot s
struct KnotAt {
    int i, k, s;
};

// tr: the terrain table and / or the weight table, or nothing (TerrT, hsddp_device.h)
template <bool EL, typename... TR>
__global__ __launch_bounds__(64) void k_simulate_policy(Params p, Bufs d, SimArgs a, TR... tr)
{
    const auto terr = terrain_of(tr...);
    __shared__ double sh[PK];
    const int chunks = (a.M + 63) / 64;
    const int b = blockIdx.x / chunks, lane = threadIdx.x, m = (blockIdx.x % chunks) * 64 + lane;
    const bool mine = m < a.M;
    const size_t row = (size_t)b * a.M + (mine ? m : a.M - 1);  // (lanes past M read the last sample, store nothing)
    const auto L = layout_of<EL>(d, b);
    const int nb = nom_buf(d, b);
    const double *Xbar = xbuf(d, nb) + (size_t)b * p.S * NX, *Ubar = ubuf(d, nb) + (size_t)b * p.Kc * NU;
    // entry e = lane + 64 t of knot kc's rows (zero past PK)
    auto fetch = [&](int kc, const KnotAt &at, double (&pre)[PK_T]) {
        const size_t kr = ((size_t)b * p.Kc + kc) * KCW;
        const double *xr = ref_ptr(p, d.ref_x, b, at.s, NX), *ur = ref_ptr(p, d.ref_u, b, at.s, NU),
                     *pf = ref_ptr(p, d.ref_foot, b, at.s, 12);
        const double *cc = (const double *)(d.contacts + ((size_t)b * (p.P + 1) + at.i) * 4);  // (16-byte aligned rows)
#pragma unroll
        for (int t = 0; t < PK_T; ++t) {
            const int e = lane + 64 * t;
            double v = 0.0;
            if (e >= PK_K && e < PK_XR) {
                if (p.fp32) v = (double)d.K32[kr + (e - PK_K)];
                else v = d.K[kr + (e - PK_K)];
            } else if (e < PK) {
                const double *src = e < PK_UB ? Xbar + (size_t)at.s * NX + e
                                  : e < PK_K ? Ubar + (size_t)kc * NU + (e - PK_UB)
                                  : e < PK_UR ? xr + (e - PK_XR)
                                  : e < PK_PF ? ur + (e - PK_UR)
                                  : e < PK_C ? pf + (e - PK_PF)
                                             : cc + (e - PK_C);
                v = *src;
            }
            pre[t] = v;
        }
    };
    double x[NX];
    {
        const double *xi = a.x_init ? a.x_init + row * NX : d.x0 + (size_t)b * NX;
#pragma unroll
        for (int j = 0; j < NX; ++j) x[j] = xi[j];
    }
    double cost = 0.0, min_grf = __builtin_inf(), max_td = 0.0;
    int steps = 0, status = 0;
    bool live = mine;
    const int P = L.P();
    KnotAt at{0, 0, L.s0(0)};
    double pre[PK_T];
    fetch(0, at, pre);
#pragma unroll 1
    for (int kc = 0; kc < a.n_steps; ++kc) {
        if (!__any(live)) break;
        const int N = L.N(at.i), i = at.i, k = at.k, s = at.s;
        __syncthreads();  // the previous knot's reads of the stage are done
#pragma unroll
        for (int t = 0; t < PK_T; ++t)
            if (lane + 64 * t < PK) sh[lane + 64 * t] = pre[t];
        __syncthreads();
        // the next knot's place, and its rows on their way
        if (k + 1 == N) { at.i = i + 1; at.k = 0; at.s = s + 2; }
        else { at.k = k + 1; at.s = s + 1; }
        if (kc + 1 < a.n_steps) fetch(kc + 1, at, pre);
        int c[4], cn[4];
        {
            const int *cc = (const int *)(sh + PK_C);
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                c[l] = __builtin_amdgcn_readfirstlane(cc[l]);
                cn[l] = __builtin_amdgcn_readfirstlane(cc[4 + l]);
            }
        }
        if (live) {
            const double cd[4] = {(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
            const double *xb = sh + PK_XB, *ub = sh + PK_UB;
            double dx[NX], u[NU], xs[NX];
#pragma unroll
            for (int j = 0; j < NX; ++j) dx[j] = x[j] - xb[j];
            // K (X - Xbar) from the 12 coupled gain rows (KCW layout: row q is control q of a stance
            // leg, control 12 + q of a swing leg; the other rows are zero), as k_rollout_tail
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                const double *g = sh + PK_K + q * NX;
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) acc += g[j] * dx[j];
                u[q] = ub[q] + (c[q / 3] ? acc : 0.0);
                u[12 + q] = ub[12 + q] + (c[q / 3] ? 0.0 : acc);
                SFENCE();  // one gain row's stage reads beside its FMAs, not all twelve rows' up front
            }
            if (a.X && mine) {  // lane-strided rows: for inspection (include/hsddp.h)
                double *xo = a.X + (row * a.n_steps + kc) * NX, *uo = a.U + (row * a.n_steps + kc) * NU;
#pragma unroll
                for (int j = 0; j < NX; ++j) { xo[j] = x[j]; uo[j] = u[j]; }
            }
            hkd_step(x, u, cd, p.dt, xs);
            SFENCE();
            double n2 = 0.0;
#pragma unroll
            for (int j = 0; j < NX; ++j) n2 += xs[j] * xs[j];
            if (!(sqrt(n2) <= 1e6)) {  // (NaN too) the sample stops at this knot with its last accepted state
                status = 1;
                live = false;
            } else {
                const double *xr = sh + PK_XR, *ur = sh + PK_UR, *pf = sh + PK_PF;
                const auto &w = terr.w(p, b, i);  // the weights of the knot's phase
                const double lt = cost_tracking(w, c, x, xr), lu = cost_control(w, u, ur), lf = cost_foot(w, c, x, xr, pf);
                cost += cost_combine(p, c, lt, lu, lf, 0.0);  // (no ReB term)
                const double mu = terr.mu(p, b, i);
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    if (!c[l]) continue;
#pragma unroll
                    for (int r = 0; r < 5; ++r) min_grf = fmin(min_grf, grf_value(mu, r, u + 3 * l));
                }
                steps = kc + 1;
#pragma unroll
                for (int j = 0; j < NX; ++j) x[j] = xs[j];
                if (k == N - 1) {  // x is X_i[N_i]: terminal cost, touchdown heights, reset map
                    const int se = s + 1;
                    const double *xe = ref_ptr(p, d.ref_x, b, se, NX), *pe = ref_ptr(p, d.ref_foot, b, se, 12);
                    const int none[MTD] = {0, 0, 0, 0};  // (no AL term)
                    double tv;
                    const double ground = terr.ground(p, b, i);
                    cost += terminal_cost_h(p, w, c, x, xe, pe, none, nullptr, nullptr, nullptr, tv);
#pragma unroll
                    for (int l = 0; l < 4; ++l)
                        if (touchdown(c, cn, l)) max_td = fmax(max_td, fabs(hkd_foot_height_grad(l, x, nullptr) - ground));
                    if (i + 1 < P) {
                        hkd_resetmap(x, c, cn, xs);
#pragma unroll
                        for (int j = 0; j < NX; ++j) x[j] = xs[j];
                    }
                }
            }
        }
    }
    if (!mine) return;
    double *xo = a.x_end + row * NX;
#pragma unroll
    for (int j = 0; j < NX; ++j) xo[j] = x[j];
    if (a.summary) {
        hsddp_sim_sample &o = a.summary[row];
        o.cost = cost; o.min_grf = min_grf; o.max_td = max_td; o.steps = steps; o.status = status;
    }
}

void launch_simulate_policy(const Params &p, const Bufs &d, const SimArgs &a, const double *terrain, WtsTab weights,
                            hipStream_t st)
{
    const unsigned grid = (unsigned)p.B * (unsigned)((a.M + 63) / 64);
    with_flags_tables([&](auto el, auto... tr) {
        hipLaunchKernelGGL(k_simulate_policy<decltype(el)::value>, dim3(grid), dim3(64), 0, st, p, d, a, tr...);
    }, terrain, weights, p.elem_layout);
}

}  // namespace hsddp
