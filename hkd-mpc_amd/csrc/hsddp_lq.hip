// hsddp_lq.hip — the LQ model of the working trajectory and the terminal tasks (gfx950, fp64 or
// the fp32 Riccati mode's records): k_lq, k_terminal and their launcher, launch_lq.
// SinglePhase::compute_cost / LQ_approximation (SinglePhase.cpp:235-296); HKDReset.h:78-136.
#include "hsddp_device.h"
#include "hsddp_dispatch.h"

namespace hsddp {

using namespace hkd;

#ifndef FWD_MINB
#define FWD_MINB 2  // 256-thread blocks per CU for the knot-parallel k_lq
#endif

// ---------------------------------------------------------------------------------------------
// Record stores of k_lq.  One lane computes one knot's record, so direct stores from the lanes hit
// 64 records (64 cache lines) per instruction.  For the gradient pieces (lx, lu, ReB Hessian) each
// wave instead stages the piece of its records in LDS (lane-major, odd stride) and the lanes still
// active write it back record by record: consecutive lanes write consecutive 2-value pairs of one
// record, so an instruction covers ~1 KB of contiguous records.  Pieces are even-sized at even
// offsets, so every pair is aligned in HBM.  Lanes that returned early (past the batch, finished
// element, phase-end slot) left ridx = -1 and their records are skipped.
// LDS stride per lane: one 128-byte line of a record (16 fp64 / 32 fp32 values) + 1
template <typename T> constexpr int LQ_STG = 128 / (int)sizeof(T) + 1;

// the wave's staged values (record positions OFF .. OFF + N - 1 at stage columns 0 .. N - 1) to the
// records, pair by pair, by the still-active lanes
template <typename T>
DEV void lq_flush(T *wl, const long *ridx, T *lq, int ldw, int lane, int OFF, int N)
{
    wave_sync();
    using T2 = std::conditional_t<std::is_same_v<T, float>, float2, double2>;
    const unsigned long long m = __ballot(1);
    const int na = __popcll(m), rank = __popcll(m & ((1ull << lane) - 1));
    for (int q = rank; q < 64 * (N / 2); q += na) {
        const int r = q / (N / 2), jp = q % (N / 2);
        const long rr = ridx[r];
        if (rr >= 0) {
            T2 w;
            w.x = wl[r * LQ_STG<T> + 2 * jp];
            w.y = wl[r * LQ_STG<T> + 2 * jp + 1];
            *reinterpret_cast<T2 *>(lq + rr * ldw + OFF + 2 * jp) = w;
        }
    }
    wave_sync();
}

// The terminal task of one (element, phase): Phix, Phixx (+AL, quirk A4) and the reset-map
// Jacobian Px, on TERM_TL lanes — TERM_TPW tasks share a wave (the per-task work is mostly serial:
// the leg kinematics on four lanes, the cost on one), so the LDS per task, not the wave count,
// bounds how many run at once.
#ifndef HSDDP_TERM_TPW
#define HSDDP_TERM_TPW 2
#endif
constexpr int TERM_TPW = HSDDP_TERM_TPW, TERM_TL = 64 / TERM_TPW;
struct TermLds {
    double sx[NX], shx[4][NX], scoef[4][2], sh[4], sxr[NX], spf[12], ssl[2 * MTD * 4];
    double sdw[NX + 12];  // the foot Hessian's diagonal, then its cross weights; first the 15 angles' sin / cos
    double spx[12 * (NX + 1)];  // Px rows 12 .. 23 (rows 0 .. 11 are the identity's)
    int sc[4], scn[4], smask[MTD];
};
static_assert(TERM_TL >= NX && TERM_TL >= 2 * MTD * 4 && TERM_TL >= 16, "terminal lane roles");

template <bool EL, typename TR>
DEV void terminal_task(const Params &p, const Bufs &d, const TR &terr, TermLds &S, int task, int t)
{
    const int b = task / p.P, i = task % p.P;
    const ElemState &E = d.el[b];
    if (E.done || E.inner_done) return;
    const auto L = layout_of<EL>(d, b);
    const int P = L.P();
    if (i >= P) return;
    double *sx = S.sx, (*shx)[NX] = S.shx, (*scoef)[2] = S.scoef, *sh = S.sh, *sxr = S.sxr, *spf = S.spf, *ssl = S.ssl;
    int *sc = S.sc, *scn = S.scn, *smask = S.smask;
    const int s = L.s0(i) + L.N(i);
    const double *xr = ref_ptr(p, d.ref_x, b, s, NX), *pf = ref_ptr(p, d.ref_foot, b, s, 12);
    // X[N] and the terminal cost's other inputs, staged together (no memory round trip at the end)
    if (t < NX) {
        sx[t] = xbuf(d, work_buf(d, b))[((size_t)b * p.S + s) * NX + t];
        sxr[t] = xr[t];
    }
    // the phase's touchdown constraints: AL parameters [slot][leg] (sigma, then lambda) and leg masks
    if (t < 2 * MTD * 4) ssl[t] = (t < MTD * 4 ? d.al_sigma : d.al_lambda)[((size_t)b * p.P + i) * MTD * 4 + (t & (MTD * 4 - 1))];
    constexpr int MK = TERM_TL - MTD;
    if (t >= MK) smask[t - MK] = d.td_mask[((size_t)b * p.P + i) * MTD + t - MK];
    if (t >= 4 && t < 16) spf[t - 4] = pf[t - 4];
    if (t < 4) {
        const int *cc = d.contacts + ((size_t)b * (p.P + 1) + i) * 4;
        sc[t] = cc[t]; scn[t] = cc[4 + t];
    }
    wave_sync();
    // Px at X_i[N] (HKDReset.h:78-136) is built in LDS from the identity (phase boundaries only)
    double *spx = S.spx;
    const bool bnd = i < P - 1;
    for (int e = t; e < 4 * NX; e += TERM_TL) (&shx[0][0])[e] = 0.0;
    if (bnd)
        for (int e = t; e < 12 * (NX + 1); e += TERM_TL) spx[e] = (e / (NX + 1) + 12 == e % (NX + 1)) ? 1.0 : 0.0;
    // the kinematics' 15 angles, one sincos per lane: yaw, pitch, roll, then per leg q0, q1, q1 + q2
    double *strig = S.sdw;
    unsigned need = td_union(smask);
#pragma unroll
    for (int l = 0; l < 4; ++l) need |= (bnd && touchdown(sc, scn, l)) ? 1u << l : 0u;
    if (need && t < 15) {
        const int m = t - 3;
        const double a = t < 3 ? sx[t] : m % 3 == 2 ? sx[11 + m] + sx[12 + m] : sx[12 + m];
        sincos(a, &strig[2 * t], &strig[2 * t + 1]);
    }
    wave_sync();
    if (t < 4) {
        // legs of the touchdown constraints: foot height h and its gradient (non-zeros at 0..2, 5,
        // 12 + 3 l + k); legs touching down at a phase boundary: the reset map's foot-Jacobian rows
        // — from one evaluation of the leg's kinematics (hkd_foot_height_grad_sparse's and
        // hkd_foot_jacobian's expressions)
        const int l = t;
        const bool tdc = (td_union(smask) >> l) & 1, tdr = touchdown(sc, scn, l);
        double h = 0.0;
        if (tdc || (bnd && tdr)) {
            Rot R, Dy, Dp, Dr;
            const EulTrig tr{strig[1], strig[0], strig[3], strig[2], strig[5], strig[4]};
            rot_zyx(tr, R);
            rot_zyx_grad(tr, Dy, Dp, Dr);
            double pb[3], dpb[3][3];
            foot_body_trig(l, strig + 6 + 6 * l, pb, dpb);
            shx[l][0] = Dy.r[2][0] * pb[0] + Dy.r[2][1] * pb[1] + Dy.r[2][2] * pb[2];
            shx[l][1] = Dp.r[2][0] * pb[0] + Dp.r[2][1] * pb[1] + Dp.r[2][2] * pb[2];
            shx[l][2] = Dr.r[2][0] * pb[0] + Dr.r[2][1] * pb[1] + Dr.r[2][2] * pb[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) shx[l][12 + 3 * l + k] = R.r[2][0] * dpb[0][k] + R.r[2][1] * dpb[1][k] + R.r[2][2] * dpb[2][k];
            shx[l][5] = 1.0;
            h = (sx[5] + R.r[2][0] * pb[0] + R.r[2][1] * pb[1] + R.r[2][2] * pb[2]) - terr.ground(p, b, i);
            if (!tdc) {  // a reset-map leg without a constraint: no AL gradient
                h = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) shx[l][j] = 0.0;
            }
            if (bnd && tdr) {  // rows 12 + 3 l + k, k < 2: the foot Jacobian's rows; the k = 2 row is zero
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double *row = spx + (3 * l + k) * (NX + 1);
                    row[12 + 3 * l + k] = 0.0;
                    if (k == 2) continue;
                    row[0] = Dy.r[k][0] * pb[0] + Dy.r[k][1] * pb[1] + Dy.r[k][2] * pb[2];
                    row[1] = Dp.r[k][0] * pb[0] + Dp.r[k][1] * pb[1] + Dp.r[k][2] * pb[2];
                    row[2] = Dr.r[k][0] * pb[0] + Dr.r[k][1] * pb[1] + Dr.r[k][2] * pb[2];
                    row[3 + k] = 1.0;
#pragma unroll
                    for (int m = 0; m < 3; ++m)
                        row[12 + 3 * l + m] = R.r[k][0] * dpb[0][m] + R.r[k][1] * dpb[1][m] + R.r[k][2] * dpb[2][m];
                }
            }
        } else if (bnd && sc[l] && !scn[l]) {  // lift-off: rows 12 + 3 l + k zero
#pragma unroll
            for (int k = 0; k < 3; ++k) spx[(3 * l + k) * (NX + 2) + 12] = 0.0;
        }
        // AL gradient / Hessian coefficients of the leg, summed over the constraints holding it
        // (quirk A4: (sigma (1 + h) + lambda) hx hx^T, ConstraintsBase.h:374-399)
        double c0 = 0.0, c1 = 0.0;
        if (tdc && p.AL_active)
            for (int q = 0; q < MTD; ++q)
                if ((smask[q] >> l) & 1) {
                    const double sg = ssl[4 * q + l], lm = ssl[MTD * 4 + 4 * q + l];
                    const double hq = (smask[q] & TD_STALE) ? 0.0 : h;  // the constraint's stored h
                    c0 += sg * hq + lm;
                    c1 += sg * (1 + hq) + lm;
                }
        scoef[l][0] = c0;
        scoef[l][1] = c1;
        sh[l] = h;
    }
    wave_sync();
    // the robot's weights: Params / its row for compile-time fields, runtime-indexed ones in place
    const auto &w = terr.w(p, b, i);
    const auto &kp = terr.wk(b, i);
    double *rec = d.term + ((size_t)b * p.P + i) * TW;
    if (t == 0) {  // the phase's terminal cost at X[N] (SinglePhase::compute_cost's last term) for k_lq's slot sums
        double tv;
        d.slot_cost[(size_t)b * p.S + s] = terminal_cost_h(p, w, sc, sx, sxr, spf, smask, ssl, ssl + MTD * 4, sh, tv);
    }
    if (t < NX) { // Phix
        const int j = t;
        double v = kp.qf_gain * kp.qf_scale[j] * q_diag(kp, sc, j) * (sx[j] - sxr[j]);
        if (j >= 3 && j < 6) {
            for (int l = 0; l < 4; ++l) {
                int m = 3 * l + (j - 3);
                double e = (sx[12 + m] - sx[j]) - (spf[m] - sxr[j]);
                v += -(w.foot_term_grad * sc[l] * foot_weight(kp, sc, m) * e);
            }
        } else if (j >= 12) {
            int m = j - 12, l = m / 3;
            double e = (sx[j] - sx[3 + m % 3]) - (spf[m] - sxr[3 + m % 3]);
            v += w.foot_term_grad * sc[l] * foot_weight(kp, sc, m) * e;
        }
        for (int l = 0; l < 4; ++l) v += scoef[l][0] * shx[l][j];
        rec[TM_PHIX + j] = v;
    }
    // foot Hessian 20 D^T Qfoot D: weight of (leg l, axis j), entries (3 + j, 3 + j) (summed over
    // the legs in leg order), (12 + 3 l + j, 12 + 3 l + j) and, negated, the two cross entries.
    // Lane r < 24 forms diagonal entry r, lane m < 12 also the weight of joint column 12 + m
    // (runtime-indexed weights read once per phase, not once per entry); the 576 entries then
    // combine them.
    auto fw = [&](int l, int j) { return w.foot_term_grad * sc[l] * sc[l] * foot_weight(kp, sc, 3 * l + j); };
    double *sdd = S.sdw, *scw = S.sdw + NX;  // (the trig is dead: read before the last wave_sync)
    if (t < NX) {
        const int r = t;
        double v = kp.qf_gain * kp.qf_scale[r] * q_diag(kp, sc, r);
        if (r >= 3 && r < 6) {
            for (int l = 0; l < 4; ++l) v += fw(l, r - 3);
        } else if (r >= 12) {
            v += fw((r - 12) / 3, (r - 12) % 3);
        }
        sdd[r] = v;
    }
    if (t < 12) scw[t] = fw(t / 3, t % 3);
    wave_sync();
    // the AL terms of the touchdown legs only (a leg's coefficient is the same on every lane; the
    // others add exact zeros)
    bool use[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) use[l] = scoef[l][1] != 0.0;
    int r = t / NX, cidx = t % NX;  // entry e = t + TERM_TL j: (r, cidx) advance per step
    for (int e = t; e < NN; e += TERM_TL) { // Phixx
        double v = 0.0;
        if (r == cidx)
            v = sdd[r];
        else if (r >= 3 && r < 6 && cidx >= 12 && (cidx - 12) % 3 == r - 3)
            v = -scw[cidx - 12];
        else if (cidx >= 3 && cidx < 6 && r >= 12 && (r - 12) % 3 == cidx - 3)
            v = -scw[r - 12];
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (use[l]) v += scoef[l][1] * (shx[l][r] * shx[l][cidx]);
        rec[TM_PHIXX + e] = v;
        // Px rows 12 .. 23 from LDS, stored coalesced (rows 0 .. 11 are the identity's, written once
        // for every record at create: launch_init_params)
        if (bnd && r >= 12) rec[TM_PX + e] = spx[(r - 12) * (NX + 1) + cidx];
        r += TERM_TL / NX;
        cidx += TERM_TL % NX;
        if (cidx >= NX) {
            cidx -= NX;
            r += 1;
        }
    }
}

// lu + ReB gradient / Hessian of one knot (SinglePhase.cpp:380-394); the GRF constraint values from
// the control row's forces, or the older ones ovr (constraint_forces)
template <typename WT>
DEV void lq_lu_reb(const Params &p, const WT &w, double mu, const int *c, const double *u, const double *ovr, const double *ur, const double *dl,
                   const double *ep, double *lu, double *rb)
{
#pragma unroll
    for (int j = 0; j < NU; ++j) lu[j] = p.dt * r_diag(w, j) * (u[j] - ur[j]);
#pragma unroll
    for (int j = 0; j < 24; ++j) rb[j] = 0.0;
    // uniform ReB parameters (the default schedule) and per-knot ones as separate code: in the
    // uniform case no per-row (delta, eps) load and no per-row 1 / delta division is issued
    auto reb = [&](auto uniform) {
        constexpr bool U = decltype(uniform)::value;
        const double inv_du = p.grf_inv_delta;
#pragma unroll
        for (int lg = 0; lg < 4; ++lg) {
            if (!c[lg]) continue;
            double gu[3] = {0, 0, 0}, hu[6] = {0, 0, 0, 0, 0, 0};
            const double f0 = grf_force(u, ovr, 3 * lg), f1 = grf_force(u, ovr, 3 * lg + 1), f2 = grf_force(u, ovr, 3 * lg + 2);
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                double row[3], d1, d2;
                grf_row(mu, r, row);
                double g = row[0] * f0 + row[1] * f1 + row[2] * f2;
                const double dlr = U ? p.grf_delta : dl[5 * lg + r];
                reb_derivs(g, dlr, U ? inv_du : 1.0 / dlr, d1, d2);
                double e = U ? p.grf_eps : ep[5 * lg + r];
                for (int a = 0; a < 3; ++a) gu[a] += e * d1 * row[a];
                hu[0] += e * (d2 * row[0] * row[0]); hu[1] += e * (d2 * row[0] * row[1]);
                hu[2] += e * (d2 * row[0] * row[2]); hu[3] += e * (d2 * row[1] * row[1]);
                hu[4] += e * (d2 * row[1] * row[2]); hu[5] += e * (d2 * row[2] * row[2]);
            }
            for (int a = 0; a < 3; ++a) lu[3 * lg + a] += p.dt * gu[a];
            for (int a = 0; a < 6; ++a) rb[6 * lg + a] = p.dt * hu[a];
        }
    };
    if (p.ReB_active) {
        if (p.reb_uniform) reb(std::true_type{});
        else reb(std::false_type{});
    }
}

// One terminal wave: tasks (element, phase) TERM_TPW wave .. + TERM_TPW - 1 on S[0 ..]; the first
// wave also resets the iteration's counters (k_terminal's comment)
template <bool EL, typename TR>
DEV void terminal_wave(const Params &p, const Bufs &d, const TR &terr, TermLds *S, long wave, int lane)
{
    if (p.retry_cap > 0 && wave == 0 && lane == 0) *d.retry_count = 0;
    if (wave == 0)
        for (int t = lane; t < LS_LIVE; t += 64) d.ls_live[t] = 0;
    if (wave == 0 && lane < 4) d.counter[lane] = 0;
    const int h = lane / TERM_TL;
    const long task = wave * TERM_TPW + h;
    if (task < (long)p.B * p.P) terminal_task<EL>(p, d, terr, S[h], (int)task, lane % TERM_TL);
}

// ---------------------------------------------------------------------------------------------
// k_lq: per (element, state slot): cost and |Defect|^2 at the current (X, U); compact LQ model at
// control slots (SinglePhase::compute_cost + LQ_approximation, SinglePhase.cpp:235-296).
// F32: config C5's fp32 Riccati mode (records in fp32 plus an fp32 copy of Defect for the sweep)
// The A - I / B pieces go out by direct stores (staging them would keep all 102 values live).
// SLOTS: the slot costs and |Defect|^2 are recomputed (Params::lq_slots; instantiated apart so the
// common path keeps the registers the cost code would take)
// tr: the terrain table and / or the weight table, or nothing (TerrT, hsddp_device.h)
template <bool F32, bool EL, bool SLOTS, typename... TR>
__global__ __launch_bounds__(256, FWD_MINB) void k_lq(Params p, Bufs d, TR... tr)
{
    const auto terr = terrain_of(tr...);
    using T = std::conditional_t<F32, float, double>;
    // the record stage of the knot waves, or the LDS of the terminal waves (blocks after them: small
    // batches, launch_lq)
    constexpr size_t STG = sizeof(T) * 4 * 64 * LQ_STG<T>, TRM = 4 * TERM_TPW * sizeof(TermLds);
    __shared__ __attribute__((aligned(16))) char lds[STG > TRM ? STG : TRM];
    T (*stage)[64 * LQ_STG<T>] = reinterpret_cast<T (*)[64 * LQ_STG<T>]>(lds);
    __shared__ long sridx[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // one thread per control knot (the records' own order); the modes that also have work at the
    // phase-end slots — |Defect|^2 (SLOTS), the fp32 Defect copy (F32) — one per state slot
    constexpr bool BY_KNOT = !SLOTS && !F32;
    const long nunit = (long)p.B * (BY_KNOT ? p.Kc : p.S);
    const long nknot = (nunit + 255) / 256;
    if ((long)blockIdx.x >= nknot) {
        terminal_wave<EL>(p, d, terr, reinterpret_cast<TermLds *>(lds) + w * TERM_TPW, ((long)blockIdx.x - nknot) * 4 + w, lane);
        return;
    }
    sridx[w][lane] = -1; // before any early return: lanes without a record stay -1
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= nunit) return;
    const int b = (int)(gid / (BY_KNOT ? p.Kc : p.S));
    const ElemState &E = d.el[b];
    if (E.done || E.inner_done) return;
    const auto L = layout_of<EL>(d, b);
    int i, k, s;
    if constexpr (BY_KNOT) {
        const int kc0 = (int)(gid % p.Kc);
        knot_phase(L, kc0, i, k);
        if (k >= L.N(i)) return;  // (every layout has Kc knots: none past the last phase)
        s = L.s0(i) + k;
    } else {
        s = (int)(gid % p.S);
        if (s >= L.S()) return;
        slot_phase(L, s, i, k);
    }
    int c[4], cn[4];
    load_contacts(d, p, b, i, c, cn);
    double x[NX];
    const int wb = work_buf(d, b);
    const double *xg = xbuf(d, wb) + ((size_t)b * p.S + s) * NX;
#pragma unroll
    for (int j = 0; j < NX; ++j) x[j] = xg[j];
    const double *dg = dbuf(d, wb) + ((size_t)b * p.S + s) * NX;
    if (SLOTS) {  // |Defect|^2 (else the last rollout's, of this working trajectory)
        double fs = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) fs += dg[j] * dg[j];
        d.slot_feas[(size_t)b * p.S + s] = fs;
    }
    if constexpr (F32) { // the sweep's and linear rollout's fp32 copy of Defect
        float *d32 = d.def32 + ((size_t)b * p.S + s) * NX;
#pragma unroll
        for (int j = 0; j < NX; ++j) d32[j] = (float)dg[j];
    }
    const double *xr = ref_ptr(p, d.ref_x, b, s, NX), *pf = ref_ptr(p, d.ref_foot, b, s, 12);
    if (k == L.N(i)) return;  // the terminal cost: the terminal task (the same function, from its foot heights)
    const int kc = L.k0(i) + k;
    sridx[w][lane] = (long)b * p.Kc + kc;
    double u[NU];
    const double *ug = ubuf(d, wb) + ((size_t)b * p.Kc + kc) * NU;
#pragma unroll
    for (int j = 0; j < NU; ++j) u[j] = ug[j];
    // the forces of the knot's stored GRF constraint values (older ones after a diverged trial)
    const double *ovr = constraint_forces(d, E, b, kc);
    const double *ur = ref_ptr(p, d.ref_u, b, s, NU);
    const double *dl = d.reb_delta + ((size_t)b * p.Kc + kc) * 20, *ep = d.reb_eps + ((size_t)b * p.Kc + kc) * 20;
    const double mu = terr.mu(p, b, i);
    const auto &wr = terr.w(p, b, i);  // the weights of the knot's phase
    if (SLOTS) {  // the running cost (else the last rollout's: same trajectory, same parameters)
        double viol;
        d.slot_cost[(size_t)b * p.S + s] = running_cost(p, wr, mu, c, x, u, xr, ur, pf, dl, ep, viol, ovr);
    }

    // the record in the solver's Riccati precision (fp64, or fp32 in config C5's mode)
    T *lqT = F32 ? (T *)d.lq32 : (T *)d.lq;
    const int ldw = F32 ? LQW32 : LQW;
    double cd[4] = {(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
    // A - I and B pieces (record positions 0 .. 103) in position order (hkd_partial_emit): each
    // value goes to this wave's LDS stage as it is computed and the stage is stored coalesced;
    // positions 15 and 67 are the record's zero slots.
    T *wl = stage[w];
    // The record leaves in 128-byte lines (W values): every line of a record is written once,
    // whole — a line written in two pieces at different times costs a second line write (PMC:
    // 7-11 % more WRITE_SIZE than the records; 0.47 -> 0.40 ms for lq + terminal when aligned).
    // Positions 0 .. 95 (A - I and B) in emission order, a line leaving with its last value;
    // positions 96 .. 103 (the last B values) then wait in the stage for lx, lu, the ReB Hessian
    // and (fp32: the record is 192 values, 6 lines) zero padding, put in position order.
    constexpr int W = 128 / (int)sizeof(T);
    auto col = [&](int pos) -> T & { return wl[lane * LQ_STG<T> + (pos & (W - 1))]; };
    auto put = [&](int pos, double v) {  // positions >= 96, in order
        col(pos) = (T)v;
        if ((pos & (W - 1)) == W - 1) lq_flush(wl, sridx[w], lqT, ldw, lane, pos - (W - 1), W);
    };
    col(15) = 0;
    hkd_partial_emit(x, u, cd, p.dt, [&](int piece, int j, double v) {
        const int pos = piece == 0 ? LQ_SE + j : piece == 1 ? sw_at(j / 17, j % 17) : bw_at(j / 12, j % 12);
        col(pos) = (T)v;
        // a line's last value (position 15 of the first fp64 line is a zero slot; 96 .. 103 wait)
        if (pos < 96 && ((pos & (W - 1)) == W - 1 || (W == 16 && pos == 14))) {
            lq_flush(wl, sridx[w], lqT, ldw, lane, pos & ~(W - 1), W);
            if (pos == 63) col(67) = 0;  // the line holding the second zero slot starts
        }
    });
    // lx: tracking + foot regularisation (HKDCost.cpp:22-37)
    {
        double lx[NX];
#pragma unroll
        for (int j = 0; j < NX; ++j) lx[j] = p.dt * q_diag(wr, c, j) * (x[j] - xr[j]);
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            double e = (x[12 + j] - x[3 + j % 3]) - (pf[j] - xr[3 + j % 3]);
            double v = p.dt * c[j / 3] * foot_weight(wr, c, j) * e;
            lx[3 + j % 3] += -v;
            lx[12 + j] += v;
        }
#pragma unroll
        for (int j = 0; j < NX; ++j) put(LQ_LX + j, lx[j]);
    }
    // lu + ReB gradient / Hessian (SinglePhase.cpp:380-394)
    double lu[NU], rb[24];
    lq_lu_reb(p, wr, mu, c, u, ovr, ur, dl, ep, lu, rb);
#pragma unroll
    for (int j = 0; j < NU; ++j) put(LQ_LU + j, lu[j]);
#pragma unroll
    for (int j = 0; j < 24; ++j) put(LQ_RB + j, rb[j]);
    if constexpr (F32)
#pragma unroll
        for (int j = LQW; j < LQW32; ++j) put(j, 0.0);
}

// The terminal tasks, TERM_TPW per wave, two waves per block: a launch of their own (82 VGPRs,
// 4.3 KB of LDS per task: 4.5 waves per SIMD; as the tail of k_lq's launch they ran at its two).
// The first wave
// also resets the iteration's counters: the parallel-retry list of the k_riccati launch that
// follows starts empty (its only reader before then is the previous iteration's
// k_riccati_select), no element has been seen searching after any trial yet (ls_live), and
// k_count's activity counts start from zero (the graph-replayed iteration has no memset launches).
template <bool EL, typename... TR>
__global__ __launch_bounds__(128, 4) void k_terminal(Params p, Bufs d, TR... tr)
{
    __shared__ TermLds S[2 * TERM_TPW];
    const int w = threadIdx.x >> 6;
    terminal_wave<EL>(p, d, terrain_of(tr...), S + w * TERM_TPW, (long)blockIdx.x * 2 + w, threadIdx.x & 63);
}

void launch_lq(const Params &p, const Bufs &d, const double *terrain, WtsTab weights, hipStream_t st)
{
    // the terminal waves: a launch of their own (five waves per SIMD), or, for a small batch whose
    // knot and terminal blocks all fit the chip at once (C1: one robot), the blocks after k_lq's
    // knot blocks in the same launch — one launch less on the latency path
    const unsigned nterm = blocks_for((long)p.B * p.P, 4 * TERM_TPW);
    const bool merged = nterm <= 256;
    const bool by_knot = !p.lq_slots && !p.fp32;  // k_lq's grid: control knots or state slots
    if (!merged) {
        const unsigned nt2 = blocks_for((long)p.B * p.P, 2 * TERM_TPW);
        with_flags_tables([&](auto el, auto... tr) {
            hipLaunchKernelGGL(k_terminal<decltype(el)::value>, dim3(nt2), dim3(128), 0, st, p, d, tr...);
        }, terrain, weights, p.elem_layout);
    }
    const dim3 g(blocks_for((long)p.B * (by_knot ? p.Kc : p.S), 256) + (merged ? nterm : 0));
    with_flags_tables([&](auto f32, auto el, auto slots, auto... tr) {
        hipLaunchKernelGGL((k_lq<decltype(f32)::value, decltype(el)::value, decltype(slots)::value>), g, dim3(256), 0, st, p, d,
                           tr...);
    }, terrain, weights, p.fp32, p.elem_layout, p.lq_slots);
}

}  // namespace hsddp
