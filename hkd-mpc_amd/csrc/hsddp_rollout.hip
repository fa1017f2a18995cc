// hsddp_rollout.hip — the forward line search (gfx950, fp64): one trial's slot and phase-boundary
// waves (k_rollout), the non-shooting tails (k_rollout_tail), single shooting (k_rollout_ss), and the
// trial's decision with the diverged trial's fix-up (k_decide, or fused into k_rollout's launch);
// their launchers, launch_rollout and launch_decide.
// SinglePhase::hybrid_rollout (SinglePhase.cpp:181-233); MultiPhaseDDP.cpp:73-133.
#include <cstdlib>

#include "hsddp_device.h"
#include "hsddp_dispatch.h"

namespace hsddp {

using namespace hkd;

#ifndef HSDDP_STAMPS
#define HSDDP_STAMPS 0
#endif
// Diagnostic build (make stamps): s_memtime at the stage boundaries of a k_rollout slot wave (each
// after an LDS drain only: a stage's own loads are waited where they are used), the differences of
// every full slot wave added into Bufs::dbg — element 0's slots 12 .. 15 and element 1's slots 0 .. 3
// (the sweep and the linear rollout use the others) — tools/stamps.py
#if HSDDP_STAMPS
#define RSTAMP(n)                                                                             \
    do {                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        unsigned long long t_;                                                                \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        rst[n] = t_;                                                                          \
    } while (0)
#else
#define RSTAMP(n) \
    do {          \
    } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// Per-slot outputs of one rollout trial from the slot's state x = X[k], simulated state xs =
// Xsim[k] and control u = U[k] (k < N): Defect, |Defect|^2, divergence flag, running or terminal
// cost with its constraint violation and touchdown residuals (SinglePhase.cpp:196-232).
// Defect = Xsim - X, its squared norm and the divergence flag of slot s
DEV void finish_defect(const Params &p, const Bufs &d, int b, int s, int k, const double *x, const double *xs)
{
    const size_t sb = (size_t)b * p.S;
    double nrm = 0.0, fs = 0.0;
    double *Dg = dbuf(d, trial_buf(d, b)) + (sb + s) * NX;
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        nrm += xs[j] * xs[j];
        const double df = xs[j] - x[j];
        fs += df * df;
        Dg[j] = df;
    }
    d.slot_feas[sb + s] = fs;
    d.slot_div[sb + s] = (k > 0 && sqrt(nrm) > 1e6) ? 1 : 0;
}

// the terminal cost of phase i at its last slot s (x = X[N]) with its violation and touchdown
// residuals; stored: with the constraints' stored residuals (a phase the rollout did not complete),
// else as a rollout completing the phase computes them; ground: the phase's ground height
// w: the robot's weights (TerrT::w)
template <typename WT>
DEV void finish_terminal(const Params &p, const Bufs &d, const WT &w, double ground, int b, int s, int i, const int *c, const int *cn, const double *x,
                         bool stored = false)
{
    const size_t sb = (size_t)b * p.S;
    const double *xr = ref_ptr(p, d.ref_x, b, s, NX), *pf = ref_ptr(p, d.ref_foot, b, s, 12);
    double tv, h[4];
    const size_t q = ((size_t)b * p.P + i) * MTD;
    (void)cn;
    d.slot_cost[sb + s] = terminal_cost(p, w, ground, c, x, xr, pf, d.td_mask + q, d.al_sigma + q * 4, d.al_lambda + q * 4, tv, h,
                                        stored);
    d.slot_viol[sb + s] = tv;
#pragma unroll
    for (int l = 0; l < 4; ++l) d.term_h[((size_t)b * p.P + i) * 4 + l] = h[l];
}

// the running cost of control slot kc = k0(i) + k at state slot s, mu its phase's friction
// coefficient; COLS: the reference from the entry-major copy (Bufs::ref_t: lanes on consecutive slots
// read contiguous pieces)
template <bool COLS = false, typename WT>
DEV void finish_running(const Params &p, const Bufs &d, const WT &w, double mu, int b, int s, int kc, const int *c, const double *x, const double *u)
{
    if constexpr (COLS) {
        const double *dl = d.reb_delta + ((size_t)b * p.Kc + kc) * 20, *ep = d.reb_eps + ((size_t)b * p.Kc + kc) * 20;
        alignas(16) double xr[NX], ur[NU], pf[12];
        ref_from_cols(p, d, b, s, xr, ur, pf);
        double viol;
        d.slot_cost[(size_t)b * p.S + s] = running_cost(p, w, mu, c, x, u, xr, ur, pf, dl, ep, viol);
        d.slot_viol[(size_t)b * p.S + s] = viol;
        return;
    }
    const size_t sb = (size_t)b * p.S;
    const double *xr = ref_ptr(p, d.ref_x, b, s, NX), *pf = ref_ptr(p, d.ref_foot, b, s, 12);
    const double *ur = ref_ptr(p, d.ref_u, b, s, NU);
    const double *dl = d.reb_delta + ((size_t)b * p.Kc + kc) * 20, *ep = d.reb_eps + ((size_t)b * p.Kc + kc) * 20;
    double viol;
    d.slot_cost[sb + s] = running_cost(p, w, mu, c, x, u, xr, ur, pf, dl, ep, viol);
    d.slot_viol[sb + s] = viol;
}

template <typename L_, typename TR>
DEV void finish_slot(const Params &p, const Bufs &d, const TR &terr, const L_ &L, int b, int s, int i, int k, const int *c,
                     const int *cn, const double *x, const double *xs, const double *u)
{
    finish_defect(p, d, b, s, k, x, xs);
    if (k == L.N(i))
        finish_terminal(p, d, terr.w(p, b, i), terr.ground(p, b, i), b, s, i, c, cn, x);
    else
        finish_running(p, d, terr.w(p, b, i), terr.mu(p, b, i), b, s, L.k0(i) + k, c, x, u);
}

// trial tix > 0 of an inner iteration runs only when an element is still searching after trial
// tix - 1 (Bufs::ls_live, written by the previous launch; a batch with none left returns at once)
DEV bool ls_skip(const Bufs &d, int tix)
{
    if (tix <= 0 || tix > LS_LIVE) return false;
    return __builtin_amdgcn_readfirstlane(d.ls_live[tix - 1]) == 0;
}

// k_rollout: one line-search trial (eps) per (element, state slot).  All knots are shooting states
// (HKDProblem.cpp:104), so X[k] = Xbar[k] + eps dX[k] and the simulated state at k depends only on
// knot k-1: the nonlinear rollout is knot-parallel.  U = Ubar + eps du with du = dU + K dX from the
// linear rollout (equal to the reference's Ubar + eps dU + K (X - Xbar) up to rounding of X - Xbar).
//
// One wave per 64 consecutive slots.  The trial state rows it needs (its slots and the one before)
// are formed with coalesced 16-byte loads (lanes over row entries, not rows) into LDS — the output
// X rows are stored from the same pass — and each lane then reads its rows from LDS.
constexpr int RS = NX + 1;  // LDS row stride (doubles): conflict-free row-per-lane reads

// The trial's steps b + eps v.  dX, du and dU are not reset between solves (hsddp_update_problem),
// as the reference keeps its own from tick to tick: the initial rollout (eps = 0) multiplies them
// by 0 as the reference does (SinglePhase.cpp:189, 200, 216).  (A select that skipped them at
// eps = 0 cost the metric's trials 7 %: k_rollout 148.8 -> 159.7 us.)
DEV double fma_step(double eps, double v, double b) { return __builtin_fma(eps, v, b); }
DEV double add_step(double b, double eps, double v) { return b + eps * v; }
constexpr int RW = 65;      // rows per wave: 64 slots and the one before

// X_t = Xbar + eps dX for rows r0 .. r0 + RW - 1 of the [rows][24] state buffers into LDS; rows
// of inactive elements are skipped, own rows (own(r)) are stored to the element's trial buffer
// (selof(element): the element's Bufs::sel, nominal and working buffer indices)
template <typename Act, typename Own, typename Sel>
DEV void stage_trial(double *L, const Bufs &d, const double *del, long r0, long nrows, int per, double eps,
                     int lane, Act active, Own own, Sel selof)
{
    constexpr int CH = NX / 2;  // 16-byte chunks per row
#pragma unroll 1
    for (int f = lane; f < RW * CH; f += 64) {
        const int row = f / CH, cc = 2 * (f % CH);
        const long r = r0 + row;
        if (r < 0 || r >= nrows || !active((int)(r / per))) continue;
        const int q = selof((int)(r / per));
        const double *bar = xbuf(d, q & 3);
        double *out = xbuf(d, trial_of(q & 3, (q >> 2) & 3));
        typedef double d2 __attribute__((ext_vector_type(2)));
        const d2 xb = *(const d2 *)(bar + r * NX + cc), dx = *(const d2 *)(del + r * NX + cc);
        d2 v;
        v.x = fma_step(eps, dx.x, xb.x);
        v.y = fma_step(eps, dx.y, xb.y);
        L[row * RS + cc] = v.x;
        L[row * RS + cc + 1] = v.y;
        if (own(r)) *(d2 *)(out + r * NX + cc) = v;
    }
}

// The same for per >= RW: the wave's 64 slots belong to its elements bA and bB, whose activity and
// nominal buffers are known (no per-row lookups), and the loads of all chunks are issued before any
// is used.  Row r0 may be the previous element's last slot: no slot of this wave reads it (slot 0
// of an element starts from x0 or a reset map of its own rows), so it is skipped.  Rows of
// inactive elements are read (in range, harmless) but neither staged nor stored.
DEV void stage_trial2(double *L, const Bufs &d, long r0, long nrows, int per, double eps, int lane, long g0, int bA,
                      bool aA, int nA, int tA, int bB, bool aB, int nB, int tB)
{
    constexpr int CH = NX / 2, NIT = (RW * CH + 63) / 64;
    typedef double d2 __attribute__((ext_vector_type(2)));
    // the elements' nominal (read) and trial (written) buffers
    const double *barA = kxbuf(nA), *barB = kxbuf(nB), *del = d.dX;
    double *outA = kxbuf(tA), *outB = kxbuf(tB);
    d2 xb[NIT], dx[NIT];
    long rr[NIT];
    bool use[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int f = lane + 64 * it, row = f / CH, cc = 2 * (f % CH);
        const long r = r0 + row;
        const bool in = f < RW * CH && r >= 0 && r < nrows;
        const long rc = in ? r : (r0 + 1 > 0 ? r0 + 1 : 0);  // a valid row for out-of-range chunks
        const long eb = rc / per;
        const bool first = eb == bA;
        use[it] = in && (first ? aA : eb == bB && aB);
        rr[it] = rc;
        xb[it] = *(const d2 *)((first ? barA : barB) + rc * NX + cc);
        dx[it] = *(const d2 *)(del + rc * NX + cc);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        if (!use[it]) continue;
        const int f = lane + 64 * it, row = f / CH, cc = 2 * (f % CH);
        const long r = rr[it];
        d2 v;  // Xbar + eps dX as one rounding (rollout_boundary forms the same rows)
        v.x = fma_step(eps, dx[it].x, xb[it].x);
        v.y = fma_step(eps, dx[it].y, xb[it].y);
        L[row * RS + cc] = v.x;
        L[row * RS + cc + 1] = v.y;
        const bool first = r / per == bA;
        if (r >= g0) *(d2 *)((first ? outA : outB) + r * NX + cc) = v;
    }
}

// waves per SIMD k_rollout's register budget is sized for; measured: 2 (256 VGPRs, no spills)
// 0.93 ms/step forward vs 3: 1.23, 4: 1.07
#ifndef HSDDP_ROLLOUT_WAVES
#define HSDDP_ROLLOUT_WAVES 2
#endif

// trial control row r: U = Ubar + eps du, straight from global memory (the wave's 64 rows are one
// contiguous 12 KB range, so the row-per-lane loads are served by the vector L1 / L2)
DEV void trial_row(const Bufs &d, const double *Ubar, long r, double eps, double *u)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2 *ub = (const d2 *)(Ubar + r * NU), *du = (const d2 *)(d.du + r * NU);
#pragma unroll
    for (int j = 0; j < NU / 2; ++j) {
        const d2 a = ub[j], e = du[j];
        u[2 * j] = add_step(a.x, eps, e.x);
        u[2 * j + 1] = add_step(a.y, eps, e.y);
    }
}

// v of the previous lane of the wave (DPP wave_shr:1; lane 0 gets 0).  Every lane must be active.
DEV double from_prev_lane(double v)
{
    const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)__double2loint(v), 0x138, 0xf, 0xf, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)__double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double((int)hi, (int)lo);
}

// Only the state rows go through LDS (13 KB per wave); the control rows are read per lane
// (trial_row), the slot's own control row stored from registers.  With both row sets in LDS
// (26 KB per wave) only 6 waves fit a CU: 1.25 ms/step of line search vs 0.93 here.
// The phase-boundary work of one trial, one thread per (phase i, element b), i-major so that a
// wave's threads share a phase (and, in a shared-gait batch, its contacts: no divergence): the
// reset map into the phase's first slot (MultiPhaseDDP.cpp:73-81) with that slot's Defect, and the
// terminal cost at its last slot.  These run in waves of their own: inside the slot waves, a
// lane's reset map or terminal cost (foot kinematics) stalled its 63 neighbours.
template <bool EL, typename TR>
DEV void rollout_boundary(const Params &p, const Bufs &d, const TR &terr, double eps, int init, long t)
{
    if (t >= (long)p.B * p.P) return;
    const int i = (int)(t / p.B), b = (int)(t % p.B);
    const ElemState &E = d.el[b];
    if (!(init ? !E.done : E.ls_active != 0)) return;
    const auto L = layout_of<EL>(d, b);
    if (i >= L.P()) return;
    const int nb = nom_buf(d, b), s0 = L.s0(i), sN = s0 + L.N(i);
    const double *Xbar = xbuf(d, nb);
    const size_t sb = (size_t)b * p.S;
    // trial rows X = Xbar + eps dX (the slot waves' expression: the same values)
    auto trial = [&](int s, double *x) {
        const double *xb = Xbar + (sb + s) * NX, *dx = d.dX + (sb + s) * NX;
#pragma unroll
        for (int j = 0; j < NX; ++j) x[j] = fma_step(eps, dx[j], xb[j]);
    };
    int c[4], cn[4];
    load_contacts(d, p, b, i, c, cn);
    double x[NX];
    if (i > 0) {
        double xp[NX], xs[NX];
        int cp_[4], cpn[4];
        load_contacts(d, p, b, i - 1, cp_, cpn);
        trial(s0 - 1, xp);
        trial(s0, x);
        hkd_resetmap(xp, cp_, cpn, xs);
        finish_defect(p, d, b, s0, 0, x, xs);
    }
    trial(sN, x);
    finish_terminal(p, d, terr.w(p, b, i), terr.ground(p, b, i), b, sN, i, c, cn, x);
}

// WIDE: p.S >= RW (instantiated apart: a wave's 64 slots then belong to at most two elements, and
// the kernel carries only that staging path)
template <bool EL, bool WIDE, typename TR>
DEV void rollout_block(const Params &p, const Bufs &d, const TR &terr, double eps, int init, int tix)
{
    __shared__ double Xt[RW * RS];
    const int lane = threadIdx.x;
    const long total = (long)p.B * p.S;
    const long nslot = (total + 63) / 64;
    if ((long)blockIdx.x >= nslot) {  // the phase-boundary waves (after the slot waves)
        rollout_boundary<EL>(p, d, terr, eps, init, ((long)blockIdx.x - nslot) * 64 + lane);
        return;
    }
    // (every second trial walks the slot blocks from the batch's end, where the trial before's last
    // reads of the same rows may still sit in the memory-side cache)
    const long blk = (tix > 0 && (tix & 1)) ? nslot - 1 - (long)blockIdx.x : (long)blockIdx.x;
#if HSDDP_STAMPS
    unsigned long long rst[8];
#endif
    RSTAMP(0);
    const long g0 = blk * 64, gid = g0 + lane;
    const long gl = min(g0 + 63, total - 1);
    const int bA = (int)(g0 / p.S), bB = (int)(gl / p.S);
    auto act = [&](int b) { const ElemState &E = d.el[b]; return init ? !E.done : E.ls_active != 0; };
    const bool aA = act(bA), aB = act(bB);
    bool any = aA || aB;
    for (int b = bA + 1; b < bB && !any; ++b) any = act(b);
    if (!any) return;
    auto active = [&](int b) { return b == bA ? aA : b == bB ? aB : act(b); };
    const int qA = d.sel[bA], qB = d.sel[bB];
    const int nA = qA & 3, nB = qB & 3, tA = trial_of(nA, (qA >> 2) & 3), tB = trial_of(nB, (qB >> 2) & 3);
    auto selof = [&](int b) { return b == bA ? qA : b == bB ? qB : d.sel[b]; };
    auto nomof = [&](int b) { return selof(b) & 3; };
    auto trialof = [&](int b) { const int q = selof(b); return trial_of(q & 3, (q >> 2) & 3); };
    // the control row before the wave's first slot (that slot's u_prev; every other slot takes its
    // u_prev from the previous lane): lanes 0..11 load it with the state rows, stage it after them
    typedef double d2 __attribute__((ext_vector_type(2)));
    __shared__ double Up0[NU];
    d2 ua = {0, 0}, ue = {0, 0};
    bool up0 = false;
    {
        const int s0 = (int)(g0 % p.S);
        const auto L0 = layout_of<EL>(d, bA);
        int i0, k0;
        slot_phase(L0, s0, i0, k0);
        up0 = aA && s0 < L0.S() && k0 > 0 && lane < NU / 2;
        if (up0) {
            const long r = (long)bA * p.Kc + s0 - i0 - 1;
            ua = ((const d2 *)(kubuf(nA) + r * NU))[lane];
            ue = ((const d2 *)(d.du + r * NU))[lane];
        }
    }
    // every lane stays active up to the u_prev exchange: lanes without a slot of their own work on a
    // valid one (clamped) and write nothing
    const long gc = gid < total ? gid : total - 1;
    const int b = (int)(gc / p.S), s = (int)(gc % p.S);
    const auto L = layout_of<EL>(d, b);
    const bool mine = gid < total && active(b) && s < L.S();
    int i, k;
    slot_phase(L, s < L.S() ? s : L.S() - 1, i, k);
    const int nb = nomof(b), tb = trialof(b);
    const long kq = (long)b * p.Kc + s - i;  // the slot's control row (k < N)
    const long kqmax = (long)p.B * p.Kc - 1;
    const long kqr = kq < kqmax ? kq : kqmax;  // (the terminal slot's row index is clamped and unused)
    RSTAMP(1);
    const long xr0 = g0 - 1;
    if constexpr (WIDE)
        stage_trial2(Xt, d, xr0, total, p.S, eps, lane, g0, bA, aA, nA, tA, bB, aB, nB, tB);
    else
        stage_trial(Xt, d, d.dX, xr0, total, p.S, eps, lane, active, [&](long r) { return r >= g0; }, selof);
    if (up0) {
        Up0[2 * lane] = add_step(ua.x, eps, ue.x);
        Up0[2 * lane + 1] = add_step(ua.y, eps, ue.y);
    }
    __syncthreads();
    RSTAMP(2);
    int c[4], cn[4];
    load_contacts(d, p, b, i, c, cn);
    const double *x = Xt + (gc - xr0) * RS;
    // the trial control row of the slot, U = Ubar + eps du (k < N)
    double u[NU];
    trial_row(d, kubuf(nb), kqr, eps, u);
#if HSDDP_STAMPS
    asm volatile("" : "+v"(u[0]), "+v"(u[NU - 1]));
#endif
    RSTAMP(3);
    // the running cost of a control slot (the terminal cost at k = N: the boundary waves)
    if (mine && k < L.N(i)) {
        d2 *ug = (d2 *)(kubuf(tb) + kq * NU);
#pragma unroll
        for (int j = 0; j < NU / 2; ++j) ug[j] = d2{u[2 * j], u[2 * j + 1]};
        finish_running<true>(p, d, terr.w(p, b, i), terr.mu(p, b, i), b, s, L.k0(i) + k, c, x, u);
    }
    RSTAMP(4);
    // u_prev: the previous slot's control row is the previous lane's (k > 0: slot s - 1 is a
    // control slot of the same phase), lane 0's was staged
    double up[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) up[j] = from_prev_lane(u[j]);
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < NU; ++j) up[j] = Up0[j];
    // Defect rows through LDS: each slot's row replaces its own staged state row once every lane's
    // dynamics have read theirs, then the wave stores the 64 rows as one contiguous range (16-byte
    // pieces over lanes) instead of one row per lane
    __shared__ int wflag[64];
    const bool wr = mine && (k > 0 || i == 0);
    if (wr) {
        double xs[NX];
        if (k == 0) {
#pragma unroll
            for (int j = 0; j < NX; ++j) xs[j] = d.x0[(size_t)b * NX + j];
        } else {
            double cd[4] = {(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
            hkd_step(x - RS, up, cd, p.dt, xs);
        }
        wave_sync();  // (no lane writes a row before every lane's dynamics have read the previous one)
        double *xw = Xt + (gc - xr0) * RS;
        double nrm = 0.0, fs = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            nrm += xs[j] * xs[j];
            const double df = xs[j] - xw[j];
            fs += df * df;
            xw[j] = df;
        }
        const size_t q = (size_t)b * p.S + s;
        d.slot_feas[q] = fs;
        d.slot_div[q] = (k > 0 && sqrt(nrm) > 1e6) ? 1 : 0;
    } else {
        wave_sync();
    }
    RSTAMP(5);
    wflag[lane] = wr;
    const int rsplit = (int)((long)bB * p.S - g0);  // (WIDE) rows from here on are element bB's
    double *const DtA = kdbuf(tA), *const DtB = kdbuf(tB);
    wave_sync();
    typedef double d2 __attribute__((ext_vector_type(2)));
    constexpr int CH = NX / 2;
#pragma unroll 4
    for (int f = lane; f < 64 * CH; f += 64) {
        const int row = f / CH, cc = 2 * (f % CH);
        if (wflag[row]) {
            const double *src = Xt + (row + 1) * RS + cc;
            // the row's element's trial buffer (bA below rsplit, bB from it; horizons shorter than a
            // wave: the row's own element)
            double *Dt;
            if constexpr (WIDE) Dt = row >= rsplit ? DtB : DtA;
            else Dt = kdbuf(trialof((int)((g0 + row) / p.S)));
            *(d2 *)(Dt + (g0 + row) * NX + cc) = d2{src[0], src[1]};
        }
    }
#if HSDDP_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    RSTAMP(6);
    if (lane == 0) {
        unsigned long long *acc = (unsigned long long *)d.dbg;
        const int slot[7] = {12, 13, 14, 15, 16, 17, 18};  // element 0: 12 .. 15, element 1: 0 .. 2
#pragma unroll
        for (int n = 1; n <= 6; ++n) atomicAdd(acc + slot[n - 1], rst[n] - rst[n - 1]);
        atomicAdd(acc + 19, 1ull);  // waves
    }
#endif
}

// k_rollout_tail: the non-shooting states of a phase (k >= ss; HKDProblem::update leaves a new
// last phase of horizon <= 2 without shooting states) after k_rollout has handled the rest:
// SinglePhase::hybrid_rollout's sequential branch (SinglePhase.cpp:185-222), X[k] = Xsim[k]
// (X[0] = x_init when the set is empty) and U[k] = Ubar[k] + eps dU[k] + K[k] (X[k] - Xbar[k]),
// then the slot outputs of those states.  One thread per element; rare (a few states per element).
template <bool EL, typename... TR>
__global__ __launch_bounds__(64) void k_rollout_tail(Params p, Bufs d, double eps, int init, int tix, TR... tr)
{
    if (ls_skip(d, tix)) return;
    const auto terr = terrain_of(tr...);
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const ElemState &E = d.el[b];
    if (!(init ? !E.done : E.ls_active != 0)) return;
    const size_t sb = (size_t)b * p.S, kb = (size_t)b * p.Kc;
    const auto L = layout_of<EL>(d, b);
    const int nb = nom_buf(d, b), tb = trial_buf(d, b);
    const double *Xbar = xbuf(d, nb), *Ubar = ubuf(d, nb);
    double *X = xbuf(d, tb), *U = ubuf(d, tb);  // the trial's rows (k_rollout wrote the shooting ones)
    for (int i = 0; i < L.P(); ++i) {
        const int N = L.N(i), ss = L.ss(i), s0 = L.s0(i), k0 = L.k0(i);
        if (ss >= N + 1) continue;
        int c[4], cn[4];
        load_contacts(d, p, b, i, c, cn);
        const double cd[4] = {(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
        double x[NX], xs[NX], u[NU];
        if (ss == 0) { // X[0] = Xsim[0] = x_init (MultiPhaseDDP.cpp:73-81)
            if (i == 0) {
                for (int j = 0; j < NX; ++j) xs[j] = d.x0[(size_t)b * NX + j];
            } else {
                int cp_[4], cpn[4];
                load_contacts(d, p, b, i - 1, cp_, cpn);
                hkd_resetmap(X + (sb + s0 - 1) * NX, cp_, cpn, xs);
            }
        } else { // Xsim[ss] from the last shooting state and its control (written by k_rollout)
            const double *xg = X + (sb + s0 + ss - 1) * NX, *ug = U + (kb + k0 + ss - 1) * NU;
            for (int j = 0; j < NX; ++j) x[j] = xg[j];
            for (int j = 0; j < NU; ++j) u[j] = ug[j];
            hkd_step(x, u, cd, p.dt, xs);
        }
        for (int k = ss; k <= N; ++k) {
            const int s = s0 + k;
            double *xg = X + (sb + s) * NX;
            for (int j = 0; j < NX; ++j) { x[j] = xs[j]; xg[j] = xs[j]; }
            const double *up = nullptr;
            if (k < N) {
                const int kc = k0 + k;
                const double *xb = Xbar + (sb + s) * NX, *ub = Ubar + (kb + kc) * NU, *du = d.dU + (kb + kc) * NU;
                double dx[NX];
                for (int j = 0; j < NX; ++j) dx[j] = x[j] - xb[j];
                for (int j = 0; j < NU; ++j) u[j] = 0.0;
                // K (X - Xbar) from the 12 coupled gain rows (KCW layout; the other rows are zero)
                for (int q = 0; q < 12; ++q) {
                    const size_t kr = ((kb + kc) * 12 + q) * NX;
                    double acc = 0.0;
                    for (int j = 0; j < NX; ++j) acc += (p.fp32 ? (double)d.K32[kr + j] : d.K[kr + j]) * dx[j];
                    u[c[q / 3] ? q : 12 + q] = acc;
                }
                double *ug = U + (kb + kc) * NU;
                for (int j = 0; j < NU; ++j) { u[j] = add_step(ub[j], eps, du[j]) + u[j]; ug[j] = u[j]; }
                up = u;
            }
            finish_slot(p, d, terr, L, b, s, i, k, c, cn, x, xs, up);
            if (k < N) hkd_step(x, u, cd, p.dt, xs);
        }
    }
}

// k_rollout_ss: one trial with single shooting (HSDDP_OPTION::MS = false).  SinglePhase::
// hybrid_rollout (SinglePhase.cpp:181-233) then takes X[k+1] = Xsim[k+1] at every knot whatever
// SS_set says (:214-220); only a phase's first state stays a shooting state when its set holds 0
// (:187-193): X[0] = Xbar[0] + eps dX[0] (dX is not written without the linear rollout,
// MultiPhaseDDP.cpp:326-329, so it keeps its last values), else X[0] = x_init.  So phases that start
// from a shooting state are independent: one thread per (element, phase), 16 per element (four
// elements per 64-thread block), each simulating its phase's knots one after another.  Then, after
// the block's barrier, the phase-start Defects (Xsim[0] = x_init: x0 or the reset map of the
// previous phase's X[N], MultiPhaseDDP.cpp:73-81) and the phases without shooting states (a new
// last phase of <= 2 knots after a receding-horizon shift), which start from that reset map.
template <bool EL, typename TR>
DEV void ss_phase(const Params &p, const Bufs &d, const TR &terr, int b, int i, double eps, const double *x_init)
{
    const auto L = layout_of<EL>(d, b);
    const size_t sb = (size_t)b * p.S, kb = (size_t)b * p.Kc;
    const int nb = nom_buf(d, b), tb = trial_buf(d, b);
    const double *Xbar = xbuf(d, nb), *Ubar = ubuf(d, nb);
    double *X = xbuf(d, tb), *U = ubuf(d, tb);
    const int N = L.N(i), s0 = L.s0(i), k0 = L.k0(i);
    int c[4], cn[4];
    load_contacts(d, p, b, i, c, cn);
    const double cd[4] = {(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
    double x[NX], xs[NX], u[NU];
    if (x_init) {  // no shooting state: X[0] = x_init (Defect[0] = 0)
        for (int j = 0; j < NX; ++j) x[j] = x_init[j];
    } else {       // X[0] = Xbar[0] + eps dX[0] (k_rollout's expression)
        const double *xb = Xbar + (sb + s0) * NX, *dx = d.dX + (sb + s0) * NX;
        for (int j = 0; j < NX; ++j) x[j] = fma_step(eps, dx[j], xb[j]);
    }
    for (int k = 0; k <= N; ++k) {
        const int s = s0 + k;
        double *xg = X + (sb + s) * NX;
        if (k > 0)
            for (int j = 0; j < NX; ++j) x[j] = xs[j];
        for (int j = 0; j < NX; ++j) xg[j] = x[j];
        if (k > 0 || x_init) finish_defect(p, d, b, s, k, x, k > 0 ? xs : x);
        if (k == N) {
            finish_terminal(p, d, terr.w(p, b, i), terr.ground(p, b, i), b, s, i, c, cn, x);
            break;
        }
        // U = Ubar + eps dU + K (X - Xbar) (SinglePhase.cpp:200), K from the 12 coupled gain rows
        const int kc = k0 + k;
        const double *xb = Xbar + (sb + s) * NX, *ub = Ubar + (kb + kc) * NU, *du = d.dU + (kb + kc) * NU;
        double dx[NX];
        for (int j = 0; j < NX; ++j) dx[j] = x[j] - xb[j];
        for (int j = 0; j < NU; ++j) u[j] = 0.0;
        for (int q = 0; q < 12; ++q) {
            const size_t kr = ((kb + kc) * 12 + q) * NX;
            double acc = 0.0;
            for (int j = 0; j < NX; ++j) acc += (p.fp32 ? (double)d.K32[kr + j] : d.K[kr + j]) * dx[j];
            u[c[q / 3] ? q : 12 + q] = acc;
        }
        double *ug = U + (kb + kc) * NU;
        for (int j = 0; j < NU; ++j) { u[j] = add_step(ub[j], eps, du[j]) + u[j]; ug[j] = u[j]; }
        finish_running(p, d, terr.w(p, b, i), terr.mu(p, b, i), b, s, kc, c, x, u);
        hkd_step(x, u, cd, p.dt, xs);
    }
}

template <bool EL, typename... TR>
__global__ __launch_bounds__(64) void k_rollout_ss(Params p, Bufs d, double eps, int init, int tix, TR... tr)
{
    if (ls_skip(d, tix)) return;
    const auto terr = terrain_of(tr...);
    const int b = blockIdx.x * 4 + (threadIdx.x >> 4), i = threadIdx.x & 15;
    bool mine = false, shoot = false;
    if (b < p.B) {
        const ElemState &E = d.el[b];
        const auto L = layout_of<EL>(d, b);
        mine = (init ? !E.done : E.ls_active != 0) && i < L.P();
        shoot = mine && L.ss(i) > 0;
    }
    if (shoot) ss_phase<EL>(p, d, terr, b, i, eps, nullptr);
    __syncthreads();  // every phase's X[N] written (same block)
    if (!mine) return;
    const auto L = layout_of<EL>(d, b);
    const size_t sb = (size_t)b * p.S;
    const int s0 = L.s0(i);
    const double *X = xbuf(d, trial_buf(d, b));
    double xi[NX];
    if (i == 0) {
        for (int j = 0; j < NX; ++j) xi[j] = d.x0[(size_t)b * NX + j];
    } else {
        int cp_[4], cpn[4];
        load_contacts(d, p, b, i - 1, cp_, cpn);
        hkd_resetmap(X + (sb + s0 - 1) * NX, cp_, cpn, xi);
    }
    if (shoot) {
        double x[NX];
        for (int j = 0; j < NX; ++j) x[j] = X[(sb + s0) * NX + j];
        finish_defect(p, d, b, s0, 0, x, xi);
    } else {
        ss_phase<EL>(p, d, terr, b, i, eps, xi);
    }
}

// A trial whose rollout breaks the 1e6 bound (SinglePhase::hybrid_rollout, SinglePhase.cpp:205-208)
// first at state slot sbrk (= s0_i + k + 1: the state simulated from knot k of phase i): the
// reference returns there and skips every later phase (MultiPhaseDDP.cpp:83-87), so X past the
// break state, U past knot k and the Defect of phase i on keep the working rows of before the
// trial, the GRF constraint values of knot k stay those of its earlier control row, and the cost
// and feasibility that follow (:116-117) are sums over those mixed rows.  The slot kernels computed
// every slot; here the element's 16 lanes (g) copy the working rows the reference keeps into the
// trial buffer, update the stored GRF values' table (Bufs::cf_flag / cf_u: the knots before the
// break now hold the trial's values, the break knot keeps its earlier ones, the later knots are
// untouched) and recompute the slot outputs from the break knot on.  No cross-lane operation (the
// caller's lanes diverge).
template <bool EL, typename TR>
DEV void diverged_fixup(const Params &p, const Bufs &d, const TR &terr, const LayT<EL> &L, int b, int g, int sbrk)
{
    int i, ks;
    slot_phase(L, sbrk, i, ks);
    const int kb = ks - 1, s0 = L.s0(i), kcb = L.k0(i) + kb, sbb = s0 + kb, S = L.S();
    const int q = d.sel[b], nb = q & 3, wb = (q >> 2) & 3, tb = trial_of(nb, wb);
    const size_t sb = (size_t)b * p.S, kq = (size_t)b * p.Kc;
    double *XT = xbuf(d, tb), *UT = ubuf(d, tb), *DT = dbuf(d, tb);
    const double *XW = xbuf(d, wb), *UW = ubuf(d, wb), *DW = dbuf(d, wb);
    for (long e = g; e < (long)(S - sbrk) * NX; e += 16) XT[(sb + sbrk) * NX + e] = XW[(sb + sbrk) * NX + e];
    for (long e = g; e < (long)(p.Kc - kcb - 1) * NX; e += 16) UT[(kq + kcb + 1) * NX + e] = UW[(kq + kcb + 1) * NX + e];
    for (long e = g; e < (long)(S - s0) * NX; e += 16) DT[(sb + s0) * NX + e] = DW[(sb + s0) * NX + e];
    int c[4], cn[4];
    load_contacts(d, p, b, i, c, cn);
    ElemState &E = d.el[b];
    // the knots before the break were passed: their stored values are the trial's (flags cleared);
    // the break knot's stay what they were — the forces of its entry if it has one, else those of
    // its working control row (the one U[kcb] held before this trial), which becomes its entry
    int *cf = d.cf_flag + kq;
    // (while E.ovr is 0 the flags are not read and their contents are arbitrary: cleared here first)
    for (int kc = g; kc < (E.ovr ? kcb : p.Kc); kc += 16)
        if (kc != kcb) cf[kc] = 0;  // (lane 0 writes the break knot's)
    if (g == 0) {
        if (!(E.ovr && cf[kcb])) {
            for (int r = 0; r < 12; ++r) d.cf_u[(kq + kcb) * 12 + r] = UW[(kq + kcb) * NX + r];
            cf[kcb] = 1;
        }
        E.ovr = 1;
    }
    __threadfence();  // rows and table visible to the other lanes of the element
    // slot outputs over the mixed rows: |Defect|^2 of phase i on, costs from the break knot on
    int ip = i;
#pragma unroll 1
    for (int s = s0 + g; s < S; s += 16) {
        while (ip + 1 < L.P() && s >= L.s0(ip + 1)) ++ip;
        const int k = s - L.s0(ip);
        const double *dr = DT + (sb + s) * NX;
        double fs = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) fs += dr[j] * dr[j];
        d.slot_feas[sb + s] = fs;
        d.slot_div[sb + s] = 0;
        if (s < sbb) continue;
        load_contacts(d, p, b, ip, c, cn);
        // (rows read in place, not staged in registers: this rare path stays light on the decide
        // kernel's registers; the arithmetic is the slot kernels')
        const double *x = XT + (sb + s) * NX;
        if (k == L.N(ip)) {
            finish_terminal(p, d, terr.w(p, b, ip), terr.ground(p, b, ip), b, s, ip, c, cn, x, true);
            continue;
        }
        const int kc = L.k0(ip) + k;
        const double *u = UT + (kq + kc) * NU;
        const double *ovr = constraint_forces(d, E, b, kc);
        const double *xr = ref_ptr(p, d.ref_x, b, s, NX), *pf = ref_ptr(p, d.ref_foot, b, s, 12);
        const double *ur = ref_ptr(p, d.ref_u, b, s, NU);
        const double *dl = d.reb_delta + (kq + kc) * 20, *ep = d.reb_eps + (kq + kc) * 20;
        double viol;
        d.slot_cost[sb + s] = running_cost(p, terr.w(p, b, ip), terr.mu(p, b, ip), c, x, u, xr, ur, pf, dl, ep, viol, ovr);
        d.slot_viol[sb + s] = viol;
    }
}

// k_decide: reductions of one trial + merit acceptance (MultiPhaseDDP.cpp:113-133) + the
// later-termination test (:358).  16 lanes per element, one per phase: each lane sums its phase's
// slots in order, and the phase sums are added in phase order — the reference's summation order
// (compute_cost, MultiPhaseDDP.cpp:431-440; SinglePhase.cpp:235-262).  A trial whose rollout broke
// the 1e6 bound (slot_div) is rejected after its rows and slot outputs are made the reference's
// mixed ones (diverged_fixup); max_tconstr / max_pconstr then cover the phases before the break
// only (MultiPhaseDDP.cpp:83-92).
template <bool EL, typename TR>
DEV void decide_group(const Params &p, const Bufs &d, const TR &terr, double eps, int last, int init, int tix, int group,
                      const int *budget)
{
    const int lane = threadIdx.x, g = lane & 15, base = lane & ~15;
    const int b = group * 4 + (lane >> 4);
    const bool valid = b < p.B;
    const ElemState *Ep = valid ? &d.el[b] : nullptr;
    const bool act = valid && (init ? !Ep->done : Ep->ls_active);
    const auto L = layout_of<EL>(d, valid ? b : 0);
    const int P = L.P();
    constexpr int NONE = 0x7fffffff;
    double ci = 0.0, fi = 0.0, pv = 0.0, tv = 0.0;
    int kd = NONE;  // first knot of the lane's phase whose simulated state breaks the bound
    auto sums = [&]() {
        ci = 0.0; fi = 0.0; pv = 0.0; tv = 0.0;
        if (!(act && g < P)) return;
        const size_t sb = (size_t)b * p.S + L.s0(g);
        const int N = L.N(g);
        // one pass, unrolled so that the loads of several slots are in flight together (each sum
        // keeps its slot order)
#pragma unroll 10
        for (int k = 0; k < N; ++k) {
            ci += d.slot_cost[sb + k];
            pv = fmin(pv, d.slot_viol[sb + k]);
            fi += d.slot_feas[sb + k];
            kd = (d.slot_div[sb + k] && k < kd) ? k : kd;
        }
        ci += d.slot_cost[sb + N];
        fi += d.slot_feas[sb + N];
        kd = (d.slot_div[sb + N] && N < kd) ? N : kd;
        tv = d.slot_viol[sb + N];
    };
    sums();
    double cost = 0.0, feas = 0.0, max_p = 0.0, max_t = 0.0;
    int sbrk = NONE;  // the element's first breaking slot
    for (int i = 0; i < p.P; ++i)
        sbrk = min(sbrk, __shfl(kd < NONE && g < P ? L.s0(g) + kd : NONE, base + i));
    const bool dvg = act && sbrk < NONE;
    int ibrk = NONE;
    if (__builtin_amdgcn_ballot_w64(dvg)) {  // (wave-uniform: the lanes of other elements repeat their sums)
        if (dvg) diverged_fixup<EL>(p, d, terr, L, b, g, sbrk);
        __threadfence();
        kd = NONE;
        sums();
        if (dvg) {
            int ks;
            slot_phase(L, sbrk, ibrk, ks);
            if (g >= ibrk) { pv = 0.0; tv = 0.0; }  // phases from the break on: not reached
        }
    }
    if (act) {
        const ElemState &Er = d.el[b];
        // (a rollout that passed every knot computed every stored GRF value from its rows: E.ovr = 0
        // below, and the per-knot flags are not read until a fix-up sets it again)
        // the phases it completed computed their touchdown residuals
        if (Er.td_stale && g < P && g < ibrk)
            for (int j = 0; j < MTD; ++j) d.td_mask[((size_t)b * p.P + g) * MTD + j] &= ~TD_STALE;
    }
    for (int i = 0; i < p.P; ++i) {  // uniform bound (lanes g >= P add exact zeros)
        cost += __shfl(ci, base + i);
        feas += __shfl(fi, base + i);
        max_p = fmin(max_p, __shfl(pv, base + i));
        max_t = fmax(max_t, __shfl(tv, base + i));
    }
    if (!act || g != 0) return;
    ElemState &E = d.el[b];
    feas = sqrt(feas);
    E.max_p = max_p;
    E.max_t = max_t;
    if (!dvg) { E.ovr = 0; E.td_stale = 0; }  // (the stale bits cleared above)
    // one entry of the solver-info buffers (cost_buffer, dyn_feas_buffer, eqn_feas_buffer,
    // ineq_feas_buffer; MultiPhaseDDP.cpp:277-280, 368-371), float as the reference's vectors
    auto push_info = [&]() {
        if (E.hist_n < p.hcap) {
            float *hv = d.hist + ((size_t)b * p.hcap + E.hist_n) * 4;
            hv[0] = (float)E.cost; hv[1] = (float)E.feas; hv[2] = (float)E.max_t; hv[3] = (float)E.max_p;
        }
        E.hist_n += 1;
    };
    const int q = d.sel[b], nb = q & 3, tb = trial_of(nb, (q >> 2) & 3);
    if (init) {  // the initial rollout is taken (update_nominal_trajectory, MultiPhaseDDP.cpp:258)
        d.sel[b] = sel_code(tb, tb);
        E.cost = cost; E.feas = feas; E.accepted = 1;
        push_info();  // the initial information (:277-280)
        return;
    }
    E.n_ls += 1;
    const double merit = cost + E.merit_rho * feas;
    const double exp_cost = eps * E.dV1 + 0.5 * eps * eps * E.dV2;
    const double exp_merit = exp_cost - eps * E.merit_rho * E.feas_prev;
    E.cost = cost; E.feas = feas; E.merit = merit;
    bool fin = false;
    if ((merit <= E.merit_prev + p.gamma * exp_merit) && !dvg) {
        E.accepted = 1; E.ls_active = 0; fin = true;
        d.sel[b] = sel_code(tb, tb);  // the trial becomes the nominal and the working trajectory
    } else {
        // the trial's rows are the working ones (the reference's X): the next trial writes the
        // third buffer, and after the last one they stay (quirk A2)
        d.sel[b] = sel_code(nb, tb);
        if (last) { E.accepted = 0; E.ls_active = 0; E.cost = E.cost_prev; E.merit = E.merit_prev; fin = true; }
    }
    if (!fin && tix >= 0 && tix < LS_LIVE) d.ls_live[tix] = 1;  // still searching (same value from every writer)
    if (fin && p.trace && E.iters >= 1 && E.iters <= 64) {
        // diagnostic trace (HSDDP_TRACE): 16 bits per inner iteration — trials (bits 0..2), accepted
        // (3), the sweep's regularisation as round(log2 mu) + 64 (bits 4..15; 0: mu = 0)
        const double mu = E.reg * 20;  // (k_riccati leaves mu / 20, or 0 below 1e-6 / 20)
        const int code = mu > 0 ? min(4095, max(1, (int)rint(log2(mu)) + 64)) : 0;
        const unsigned long long v = (unsigned long long)((tix + 1) | (E.accepted << 3) | (code << 4)) & 0xffffull;
        const int it = E.iters - 1;
        d.dbg[(size_t)b * 16 + it / 4] |= v << (16 * (it % 4));
    }
    if (fin) {
        // the later-termination test breaks before the iteration's entry is buffered (:358-371)
        if (!p.no_early_exit && fabs((E.cost_prev - E.cost) / E.cost_prev) < p.cost_thresh && E.feas <= p.feas_thresh)
            E.inner_done = 1;
        else
            push_info();
        // the element's own inner bound (MultiPhaseDDP.cpp:304): its last iteration of this outer one
        E.inner_n += 1;
        if (budget && E.inner_n >= budget[2 * b + 1]) E.inner_done = 1;
    }
}

// (six waves per SIMD as before the divergence path: that rare path spills instead)
template <bool EL, typename... TR>
__global__ __launch_bounds__(64) void k_decide(Params p, Bufs d, double eps, int last,
                                                                                         int init, int tix, const int *budget, TR... tr)
{
    if (ls_skip(d, tix)) return;
    decide_group<EL>(p, d, terrain_of(tr...), eps, last, init, tix, blockIdx.x, budget);
}

// One line-search trial: the slot and boundary blocks (rollout_block), and — FUSE, small batches
// without non-shooting tails (launch_rollout) — the trial's decision by the last block to finish:
// every block publishes its slot outputs (device-scope release) and takes a ticket; the block
// holding the last ticket (acquire) runs k_decide's work for the batch, four elements at a time,
// and resets the ticket counter.  One launch less per trial on the latency path of C1.
template <bool EL, bool FUSE, bool WIDE, typename... TR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HSDDP_ROLLOUT_WAVES))) void k_rollout(
    Params p, Bufs d, double eps, int init, int tix, int last, const int *budget, TR... tr)
{
    if (ls_skip(d, tix)) return;
    const auto terr = terrain_of(tr...);
    rollout_block<EL, WIDE>(p, d, terr, eps, init, tix);
    if constexpr (FUSE) {
        __shared__ int ticket;
        __threadfence();
        if (threadIdx.x == 0) ticket = atomicAdd(&d.counter[7], 1);
        __syncthreads();
        if (ticket != (int)gridDim.x - 1) return;
        __threadfence();
        for (int q = 0; q < (p.B + 3) / 4; ++q) decide_group<EL>(p, d, terr, eps, last, init, tix, q, budget);
        if (threadIdx.x == 0) d.counter[7] = 0;
    }
}

// Trajectory::update_nominal_vals (TrajectoryManagement.cpp:110-115) is k_decide's flip of
// Bufs::sel: the accepted trial's buffer becomes the nominal one, no rows are copied.  (Defect_bar
// is never read by the solver, MultiPhaseDDP.cpp / SinglePhase.cpp, and is not kept.)

// small batches without non-shooting tails decide each trial in its rollout launch (k_rollout FUSE);
// HSDDP_NO_FUSED_DECIDE=1 (read at every launch: a test switches it in-process) keeps k_decide's
// launch, for the equality test of the two paths
static bool fused_decide(const Params &p)
{
    if (p.B > 16 || p.has_tail || p.ms0) return false;
    const char *e = std::getenv("HSDDP_NO_FUSED_DECIDE");
    return !(e && *e && *e != '0');
}

void launch_rollout(const Params &p, const Bufs &d, double eps, int last, int init, int tix, const int *budget,
                    const double *terrain, WtsTab weights, hipStream_t st)
{
    if (p.ms0) {  // single shooting: every knot simulated (k_rollout_ss)
        with_flags_tables([&](auto el, auto... tr) {
            hipLaunchKernelGGL(k_rollout_ss<decltype(el)::value>, dim3((p.B + 3) / 4), dim3(64), 0, st, p, d, eps, init, tix, tr...);
        }, terrain, weights, p.elem_layout);
        return;
    }
    // slot waves, then the phase-boundary waves (k_rollout, rollout_boundary)
    const dim3 g(blocks_for((long)p.B * p.S, 64) + blocks_for((long)p.B * p.P, 64));
    const bool wide = p.S >= RW;  // (rollout_block)
    with_flags_tables([&](auto el, auto fuse, auto wd, auto... tr) {
        hipLaunchKernelGGL((k_rollout<decltype(el)::value, decltype(fuse)::value, decltype(wd)::value>), g, dim3(64), 0, st, p, d,
                           eps, init, tix, last, budget, tr...);
    }, terrain, weights, p.elem_layout, fused_decide(p), wide);
    // (a fused launch has no tail: fused_decide)
    if (p.has_tail)
        with_flags_tables([&](auto el, auto... tr) {
            hipLaunchKernelGGL(k_rollout_tail<decltype(el)::value>, dim3((p.B + 63) / 64), dim3(64), 0, st, p, d, eps, init, tix,
                               tr...);
        }, terrain, weights, p.elem_layout);
}
void launch_decide(const Params &p, const Bufs &d, double eps, int last, int init, int tix, const int *budget,
                   const double *terrain, WtsTab weights, hipStream_t st)
{
    if (fused_decide(p)) return;  // decided by the rollout launch
    with_flags_tables([&](auto el, auto... tr) {
        hipLaunchKernelGGL(k_decide<decltype(el)::value>, dim3((p.B + 3) / 4), dim3(64), 0, st, p, d, eps, last, init, tix, budget,
                           tr...);
    }, terrain, weights, p.elem_layout);
}

}  // namespace hsddp
