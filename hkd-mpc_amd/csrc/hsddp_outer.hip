// hsddp_outer.hip — the small kernels around the inner iteration (gfx950), with their launchers:
// the outer loop's AL / ReB updates and convergence tests (ConstraintsBase.h:168-183, 349-365;
// MultiPhaseDDP.cpp:383-408) and the element-state housekeeping — buffer normalisation, resets,
// parameter and touchdown-mask setup, reference columns, counts and broadcasts.
#include "hsddp_device.h"
#include "hsddp_dispatch.h"

namespace hsddp {

using namespace hkd;

// one element's nominal rows into buffer 0 (a swap of buffer 0 with the nominal's, rows of X, U and
// Defect): host downloads and uploads see Xbar / Ubar in buffer 0; sel is fixed up by k_normalize_sel
__global__ __launch_bounds__(256) void k_normalize(Params p, Bufs d)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)p.S * (NX / 2);
    if (gid >= (long)p.B * per) return;
    const int b = (int)(gid / per);
    const int nb = nom_buf(d, b);
    if (nb == 0) return;
    auto swap2 = [&](double *a0, double *a1, long at) {
        double2 *x0 = reinterpret_cast<double2 *>(a0), *x1 = reinterpret_cast<double2 *>(a1);
        const double2 t = x0[at];
        x0[at] = x1[at];
        x1[at] = t;
    };
    swap2(xbuf(d, 0), xbuf(d, nb), gid);
    swap2(dbuf(d, 0), dbuf(d, nb), gid);
    const long r = gid % per;
    if (r < (long)p.Kc * (NU / 2)) swap2(ubuf(d, 0), ubuf(d, nb), (long)b * p.Kc * (NU / 2) + r);
}
__global__ void k_normalize_sel(Params p, Bufs d)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const int nb = nom_buf(d, b), wb = work_buf(d, b);
    if (nb == 0) return;
    // nominal now in 0; buffers 0 and nb traded their rows, the working index follows its rows
    d.sel[b] = sel_code(0, wb == nb ? 0 : wb == 0 ? nb : wb);
}

// the working trajectory back at the nominal one (X = Xbar, U = Ubar) with a zero Defect, rows left
// where they are: first the nominal buffer's Defect rows are zeroed (k_reset_defect), then the
// working index follows the nominal (k_reset_sel)
__global__ __launch_bounds__(256) void k_reset_defect(Params p, Bufs d)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)p.S * (NX / 2);
    if (gid >= (long)p.B * per) return;
    reinterpret_cast<double2 *>(dbuf(d, nom_buf(d, (int)(gid / per))))[gid] = double2{0.0, 0.0};
}
__global__ void k_reset_sel(Params p, Bufs d)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < p.B) d.sel[b] = sel_code(nom_buf(d, b), nom_buf(d, b));
}

__global__ void k_outer_begin(Params p, Bufs d, const int *budget)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    ElemState &E = d.el[b];
    if (E.done) return;
    // the element's own outer bound (MultiPhaseDDP.cpp:257): no outer iteration at all
    if (budget && E.outer_iters >= budget[2 * b]) { E.done = 1; return; }
    E.outer_iters += 1;
    E.max_t_prev = E.max_t;
    E.max_p_prev = E.max_p;
    E.reg = 0.0;
    E.inner_done = (budget && budget[2 * b + 1] <= 0) ? 1 : 0;  // (an inner bound of 0: no iteration)
    E.inner_n = 0;
}

// update_REB_params (ConstraintsBase.h:168-183) per (element, control slot)
template <bool EL, typename... TR>
__global__ __launch_bounds__(256) void k_reb_update(Params p, Bufs d, TR... tr)
{
    const auto terr = terrain_of(tr...);
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)p.B * p.Kc) return;
    const int b = (int)(gid / p.Kc), kc = (int)(gid % p.Kc);
    if (d.el[b].done) return;
    const auto L = layout_of<EL>(d, b);
    int i = 0;
    for (int j = 1; j < L.P(); ++j)
        if (kc >= L.k0(j)) i = j;
    int c[4], cn[4];
    load_contacts(d, p, b, i, c, cn);
    const double *u = ubuf(d, work_buf(d, b)) + gid * NU;
    // the knot's stored GRF constraint values: from the control row, or older forces
    const double *ovr = constraint_forces(d, d.el[b], b, kc);
    double *dl = d.reb_delta + gid * 20, *ep = d.reb_eps + gid * 20;
    const double mu = terr.mu(p, b, i);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (!c[l]) continue;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const double f[3] = {grf_force(u, ovr, 3 * l), grf_force(u, ovr, 3 * l + 1), grf_force(u, ovr, 3 * l + 2)};
            double g = grf_value(mu, r, f);
            if (g > -p.pconstr_thresh) continue;
            ep[5 * l + r] *= p.update_ReB;
            dl[5 * l + r] *= p.update_relax;
            dl[5 * l + r] = fmax(dl[5 * l + r], p.grf_delta_min);
        }
    }
}

// update_AL_params (ConstraintsBase.h:349-365) + outer convergence tests (MultiPhaseDDP.cpp:397-408)
template <bool EL>
__global__ void k_outer_end(Params p, Bufs d, const int *budget)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    ElemState &E = d.el[b];
    if (E.done) return;
    if (p.AL_active) {
        const int P = layout_of<EL>(d, b).P();
        // TerminalConstraintBase::update_params (ConstraintsBase.h:354-372) of every touchdown
        // constraint of every phase, leg by leg
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < MTD; ++j) {
                const int m = d.td_mask[((size_t)b * p.P + i) * MTD + j];
                for (int l = 0; l < 4; ++l) {
                    if (!((m >> l) & 1)) continue;
                    // the constraint's stored h: 0 when never computed since it was registered
                    const double h = (m & TD_STALE) ? 0.0 : d.term_h[((size_t)b * p.P + i) * 4 + l];
                    const size_t q = (((size_t)b * p.P + i) * MTD + j) * 4 + l;
                    if (fabs(h) < p.tconstr_thresh) continue;
                    if (fabs(h) > 0.005) {
                        d.al_sigma[q] *= p.update_penalty;
                        d.al_sigma[q] = fmin(d.al_sigma[q], p.td_sigma_max);
                    } else {
                        d.al_lambda[q] += h * d.al_sigma[q];
                    }
                }
            }
    }
    // the element's own outer bound: that was its last outer iteration (its AL / ReB update done)
    if (budget && E.outer_iters >= budget[2 * b]) E.done = 1;
    if (p.no_early_exit) return;
    if (E.max_t < p.tconstr_thresh && fabs(E.max_p) < p.pconstr_thresh && E.feas <= p.feas_thresh) E.done = 1;
    else if (fabs(E.max_t - E.max_t_prev) < 0.0001 && fabs(E.max_p - E.max_p_prev) < 0.0001 &&
             E.feas <= p.feas_thresh)
        E.done = 1;
}

__global__ void k_reset_elements(Params p, Bufs d)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    ElemState &E = d.el[b];
    const int ovr = E.ovr, tds = E.td_stale;  // (the constraint objects outlive the solve)
    E = ElemState{};
    E.ovr = ovr;
    E.td_stale = tds;
}

__global__ __launch_bounds__(256) void k_init_params(Params p, Bufs d)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < (long)p.B * p.Kc * 20) { d.reb_delta[gid] = p.grf_delta; d.reb_eps[gid] = p.grf_eps; }
    if (gid < (long)p.B * p.P * MTD * 4) { d.al_sigma[gid] = p.td_sigma; d.al_lambda[gid] = p.td_lambda; }
    // one touchdown constraint per phase towards the next phase's contact (HKDProblem::
    // initialization's add_tconstr_one_phase, HKDProblem.cpp:104), resolved from the contact rows
    if (gid < (long)p.B * p.P * MTD) d.td_mask[gid] = gid % MTD == 0 ? TD_PENDING | TD_STALE : 0;
    // a new problem's constraint values are zero (create_data, ConstraintsBase.h:26-34, 50-54):
    // every knot's GRF values from zero forces, every touchdown h zero (TD_STALE above)
    if (gid < (long)p.B * p.Kc * 12) d.cf_u[gid] = 0.0;
    if (gid < (long)p.B * p.Kc) d.cf_flag[gid] = 1;
    if (gid < (long)p.B) { d.el[gid].ovr = 1; d.el[gid].td_stale = 1; }
}

// Px rows 0 .. 11 of every terminal record slot (the allocation's B x MAXP, whatever the
// layout): the reset map leaves the orientation, position and velocity rows as the identity's
// (HKDReset.h:78-136), so k_terminal writes only rows 12 .. 23
__global__ __launch_bounds__(256) void k_term_identity(Params p, Bufs d)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)p.B * MAXP * 12 * NX) return;
    const long rec = gid / (12 * NX);
    const int e = (int)(gid % (12 * NX));
    d.term[rec * TW + TM_PX + e] = (e / NX == e % NX) ? 1.0 : 0.0;
}

// TD_PENDING slots take the touchdown legs of their phase's contact rows (0: no constraint)
template <bool EL>
__global__ __launch_bounds__(256) void k_resolve_td(Params p, Bufs d)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)p.B * p.P * MTD) return;
    const int b = (int)(gid / ((long)p.P * MTD)), i = (int)(gid / MTD % p.P);
    int &m = d.td_mask[gid];
    if (i >= layout_of<EL>(d, b).P()) { m = 0; return; }
    if (!(m & TD_PENDING)) return;
    int c[4], cn[4];
    load_contacts(d, p, b, i, c, cn);
    const int legs = td_bits(c, cn);
    m = legs ? legs | (m & TD_STALE) : 0;
}

// The caller's touchdown leg masks [B][P][MTD] (hsddp_upload_constraint_params) merged into the
// device's: a slot whose legs are unchanged is the same constraint object and keeps its TD_STALE /
// TD_PENDING bits (the caller never sees them); a slot that goes to 0 is cleared; any other is a new
// constraint object, whose residual reads 0 until a rollout computes it.
__global__ __launch_bounds__(256) void k_upload_td(Params p, Bufs d, const int *legs)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)p.B * p.P * MTD) return;
    const int old = d.td_mask[gid], nl = legs[gid] & 15;
    if ((old & 15) == nl) return;
    d.td_mask[gid] = nl ? nl | TD_STALE : 0;
    if (nl) d.el[gid / ((long)p.P * MTD)].td_stale = 1;
}

// Bufs::ref_t: one thread per (entry j, column r), j-major so that the column stores are contiguous
__global__ __launch_bounds__(256) void k_ref_columns(Bufs d, long ncol)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= ncol * REF_COLS) return;
    const int j = (int)(gid / ncol);
    const long r = gid % ncol;
    const double v = j < NX ? d.ref_x[r * NX + j] : j < NX + NU ? d.ref_u[r * NU + j - NX] : d.ref_foot[r * 12 + j - NX - NU];
    d.ref_t[((size_t)(j >> 1) * d.ref_tw + r) * 2 + (j & 1)] = v;
}

void launch_ref_columns(const Params &p, const Bufs &d, int Bref, hipStream_t st)
{
    const long ncol = (long)Bref * p.S, n = ncol * REF_COLS;
    hipLaunchKernelGGL(k_ref_columns, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, ncol);
}

// which: 0 = elements with ls_active, 1 = elements still iterating (!done && !inner_done), 2 = !done
__global__ void k_count(Params p, Bufs d, int which)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int v = 0;
    if (b < p.B) {
        const ElemState &E = d.el[b];
        v = which == 0 ? E.ls_active : which == 1 ? (!E.done && !E.inner_done) : !E.done;
    }
    unsigned long long m = __ballot(v);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&d.counter[which], __popcll(m));
}

// sums of n_ls and iters over the elements into counter[4], counter[5] (hsddp_stats)
__global__ void k_stat_sums(Params p, Bufs d)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int a = 0, c = 0;
    if (b < p.B) {
        a = d.el[b].n_ls;
        c = d.el[b].iters;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        c += __shfl_xor(c, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&d.counter[4], a);
        atomicAdd(&d.counter[5], c);
    }
}

__global__ __launch_bounds__(256) void k_broadcast(double *dst, const double *src, size_t n, size_t total)
{
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < total) dst[gid] = src[gid % n];
}
void launch_broadcast(double *dst, const double *src, size_t n, size_t copies, hipStream_t st)
{
    const size_t total = n * copies;
    if (total) hipLaunchKernelGGL(k_broadcast, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dst, src, n, total);
}

void launch_normalize(const Params &p, const Bufs &d, hipStream_t st)
{
    hipLaunchKernelGGL(k_normalize, dim3(blocks_for((long)p.B * p.S * (NX / 2), 256)), dim3(256), 0, st, p, d);
    hipLaunchKernelGGL(k_normalize_sel, dim3(blocks_for(p.B, 256)), dim3(256), 0, st, p, d);
}
void launch_reset_working(const Params &p, const Bufs &d, hipStream_t st)
{
    hipLaunchKernelGGL(k_reset_defect, dim3(blocks_for((long)p.B * p.S * (NX / 2), 256)), dim3(256), 0, st, p, d);
    hipLaunchKernelGGL(k_reset_sel, dim3(blocks_for(p.B, 256)), dim3(256), 0, st, p, d);
}
void launch_outer_begin(const Params &p, const Bufs &d, const int *budget, hipStream_t st)
{
    hipLaunchKernelGGL(k_outer_begin, dim3(blocks_for(p.B, 256)), dim3(256), 0, st, p, d, budget);
}
void launch_reb_update(const Params &p, const Bufs &d, const double *terrain, hipStream_t st)
{
    with_flags_table([&](auto el, auto... tr) {
        hipLaunchKernelGGL(k_reb_update<decltype(el)::value>, dim3(blocks_for((long)p.B * p.Kc, 256)), dim3(256), 0, st, p, d, tr...);
    }, terrain, p.elem_layout);
}
void launch_outer_end(const Params &p, const Bufs &d, const int *budget, hipStream_t st)
{
    with_flags([&](auto el) {
        hipLaunchKernelGGL(k_outer_end<decltype(el)::value>, dim3(blocks_for(p.B, 256)), dim3(256), 0, st, p, d, budget);
    }, p.elem_layout);
}
void launch_reset_elements(const Params &p, const Bufs &d, hipStream_t st)
{
    hipLaunchKernelGGL(k_reset_elements, dim3(blocks_for(p.B, 256)), dim3(256), 0, st, p, d);
}
void launch_init_params(const Params &p, const Bufs &d, hipStream_t st)
{
    long n = (long)p.B * p.Kc * 20;
    if ((long)p.B * p.P * MTD * 4 > n) n = (long)p.B * p.P * MTD * 4;
    hipLaunchKernelGGL(k_init_params, dim3(blocks_for(n, 256)), dim3(256), 0, st, p, d);
    hipLaunchKernelGGL(k_term_identity, dim3(blocks_for((long)p.B * MAXP * 12 * NX, 256)), dim3(256), 0, st, p, d);
}
void launch_resolve_td(const Params &p, const Bufs &d, hipStream_t st)
{
    with_flags([&](auto el) {
        hipLaunchKernelGGL(k_resolve_td<decltype(el)::value>, dim3(blocks_for((long)p.B * p.P * MTD, 256)), dim3(256), 0, st, p, d);
    }, p.elem_layout);
}
void launch_upload_td(const Params &p, const Bufs &d, const int *legs, hipStream_t st)
{
    hipLaunchKernelGGL(k_upload_td, dim3(blocks_for((long)p.B * p.P * MTD, 256)), dim3(256), 0, st, p, d, legs);
}
void launch_stat_sums(const Params &p, const Bufs &d, hipStream_t st)
{
    hipLaunchKernelGGL(k_stat_sums, dim3((p.B + 255) / 256), dim3(256), 0, st, p, d);
}

void launch_count(const Params &p, const Bufs &d, int which, hipStream_t st)
{
    hipLaunchKernelGGL(k_count, dim3(blocks_for(p.B, 256)), dim3(256), 0, st, p, d, which);
}

}  // namespace hsddp
