// hsddp_restart.hip — single elements of a live handle started again as new problems
// (hsddp_restart_elements): HKDProblem::initialization (HKDProblem.cpp:15-111) for a subset of the
// batch, i.e. what HKDMPCSolver::initialize builds for one robot (HKDMPC.cpp:20-94) while the other
// robots stay in their HKDMPCSolver::update (:97-166).
//
// The restarted elements come as a compacted list, and every kernel's grid is (work of one
// element) x (listed elements): the cost follows the number of restarted elements, not B.  Each
// writes what hsddp_upload_problem + hsddp_upload_warm_start(h, NULL, NULL, NULL) leave of a new
// problem's element and nothing of any other element:
//
//   k_restart_slots   per state slot: the reference rows and entry-major columns (k_build_refs'
//                     arithmetic, HKDReference.cpp:8-57), Xbar = X = ref_x in buffer 0
//                     (HKDProblem.cpp:84-90), Defect = dX = 0, the fp32 Defect copy, the slot sums
//   k_restart_knots   per control slot: K = 0 (whole 128-byte lines), Ubar = U = dU = du = 0, the
//                     ReB pair of every GRF row, the stored GRF values (zero forces, cf_flag = 1),
//                     the fp32 LQ records
//   k_restart_elem    per element: buffer selector, ElemState (with the solver-info count), one
//                     touchdown constraint per phase with the initial AL parameters, the stored
//                     touchdown values, the contact rows and x0
//
// The row stores are 16 bytes wide and consecutive lanes store consecutive pieces of a row.  The
// entry-major reference columns (Bufs::ref_t) are written by the same lanes, 16 bytes each at the
// column's stride: 480 of a slot's 1564 bytes go out as single pieces, which at a restart's volume
// costs nothing measurable.
#include "hsddp_device.h"
#include "hsddp_mpc.h"
#include "hsddp_restart.h"

namespace hsddp {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

// 16-byte pieces of one state slot: ref_x 12, ref_u 12, ref_foot 6
constexpr int SLOT_U = NX / 2 + NU / 2 + 6;

// One thread per (listed element, state slot, piece).  Piece u < 12 holds entries 2u, 2u + 1 of
// ref_x (and of the Xbar, Defect and dX rows), 12 <= u < 24 of ref_u, the last six of ref_foot
// (and four values each of the fp32 Defect row).
__global__ __launch_bounds__(256) void k_restart_slots(Params p, Bufs d, RestartArgs a)
{
    const long per = (long)p.S * SLOT_U, gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)a.n * per) return;
    const int m = (int)(gid / per), s = (int)(gid % per / SLOT_U), u = (int)(gid % SLOT_U);
    const size_t b = (size_t)a.list[m], row = b * p.S + s;
    if (u < NX / 2) {
        d2 v;
        if (a.build_refs) {
            int k = a.start[m] + a.slot_idx[(size_t)a.map_id[m] * p.S + s];
            k = k < a.table_n ? k : a.table_n - 1;  // past the loaded data: its last sample
            const double *q = a.table + (size_t)k * RT_W;
            const int j = 2 * u;
            if (j < 12) v = d2{q[RT_BODY + j], q[RT_BODY + j + 1]};
            else {  // foot placement of a stance leg, joint angles of a swing leg (entry by entry)
                const int e0 = j - 12, e1 = j - 11;
                v = d2{q[RT_C + e0 / 3] > 0 ? q[RT_FOOT + e0] : q[RT_QJ + e0],
                       q[RT_C + e1 / 3] > 0 ? q[RT_FOOT + e1] : q[RT_QJ + e1]};
            }
            ((d2 *)d.ref_x)[row * (NX / 2) + u] = v;
            ((d2 *)d.ref_t)[(size_t)u * d.ref_tw + row] = v;
        } else {
            v = ((const d2 *)d.ref_x)[(size_t)s * (NX / 2) + u];  // the shared reference's row
        }
        ((d2 *)xbuf(d, 0))[row * (NX / 2) + u] = v;
        ((d2 *)dbuf(d, 0))[row * (NX / 2) + u] = d2{0.0, 0.0};
        ((d2 *)d.dX)[row * (NX / 2) + u] = d2{0.0, 0.0};
        return;
    }
    if (u < NX / 2 + NU / 2) {
        if (!a.build_refs) return;
        const int w = u - NX / 2, j = 2 * w;
        int k = a.start[m] + a.slot_idx[(size_t)a.map_id[m] * p.S + s];
        k = k < a.table_n ? k : a.table_n - 1;
        const double *q = a.table + (size_t)k * RT_W;
        const d2 v = j < 12 ? d2{q[RT_GRF + j], q[RT_GRF + j + 1]} : d2{q[RT_QJD + j - 12], q[RT_QJD + j - 11]};
        ((d2 *)d.ref_u)[row * (NU / 2) + w] = v;
        ((d2 *)d.ref_t)[(size_t)u * d.ref_tw + row] = v;
        return;
    }
    const int w = u - NX / 2 - NU / 2;
    if (p.fp32) ((f4 *)d.def32)[row * 6 + w] = f4{0.f, 0.f, 0.f, 0.f};
    if (w == 0) {  // the slot's partial sums: recomputed by the next k_lq, zero as a new handle's
        d.slot_cost[row] = 0.0;
        d.slot_feas[row] = 0.0;
        d.slot_viol[row] = 0.0;
        d.slot_div[row] = 0;
    }
    if (!a.build_refs) return;
    int k = a.start[m] + a.slot_idx[(size_t)a.map_id[m] * p.S + s];
    k = k < a.table_n ? k : a.table_n - 1;
    const double *q = a.table + (size_t)k * RT_W;
    const d2 v = d2{q[RT_FOOT + 2 * w], q[RT_FOOT + 2 * w + 1]};
    ((d2 *)d.ref_foot)[row * 6 + w] = v;
    ((d2 *)d.ref_t)[(size_t)u * d.ref_tw + row] = v;
}

// 16-byte pieces of one control slot beside its gain rows: Ubar, dU, du 12 each, the ReB delta and
// eps rows 10 each, the stored forces 6; the fp32 LQ record 48 more
constexpr int KNOT_U = 3 * (NU / 2) + 2 * 10 + 6, KNOT_U32 = KNOT_U + LQW32 / 4;

// m0 + blockIdx.y: the listed element (the grid's y extent holds 65535).  The first threads of an
// element's x range zero its compact gain rows piece by piece — one contiguous run of Kc x 18
// (fp32: 9) whole lines, every wave storing eight whole lines — the others take one piece each of
// the control slots' other rows.
template <typename KT>
__global__ __launch_bounds__(256) void k_restart_knots(Params p, Bufs d, RestartArgs a, KT *K, int m0)
{
    constexpr int KV = 16 / sizeof(KT), KU = sizeof(KT) == 4 ? KNOT_U32 : KNOT_U;
    const long nk = (long)p.Kc * KCW / KV, t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t b = (size_t)a.list[m0 + blockIdx.y];
    if (t < nk) {
        ((f4 *)(K + b * p.Kc * KCW))[t] = f4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const long e = t - (nk + 255) / 256 * 256;  // (the gain rows' last block is theirs alone)
    if (e < 0 || e >= (long)p.Kc * KU) return;
    const int kc = (int)(e / KU);
    int u = (int)(e % KU);
    const size_t q = b * p.Kc + kc;
    const d2 z = d2{0.0, 0.0};
    if (u < NU / 2) { ((d2 *)ubuf(d, 0))[q * (NU / 2) + u] = z; return; }
    u -= NU / 2;
    if (u < NU / 2) { ((d2 *)d.dU)[q * (NU / 2) + u] = z; return; }
    u -= NU / 2;
    if (u < NU / 2) { ((d2 *)d.du)[q * (NU / 2) + u] = z; return; }
    u -= NU / 2;
    if (u < 10) { ((d2 *)d.reb_delta)[q * 10 + u] = d2{p.grf_delta, p.grf_delta}; return; }
    u -= 10;
    if (u < 10) { ((d2 *)d.reb_eps)[q * 10 + u] = d2{p.grf_eps, p.grf_eps}; return; }
    u -= 10;
    if (u < 6) {
        ((d2 *)d.cf_u)[q * 6 + u] = z;
        if (u == 0) d.cf_flag[q] = 1;
        return;
    }
    u -= 6;
    if constexpr (sizeof(KT) == 4) ((f4 *)d.lq32)[q * (LQW32 / 4) + u] = f4{0.f, 0.f, 0.f, 0.f};
}

// One wave per listed element.
__global__ __launch_bounds__(64) void k_restart_elem(Params p, Bufs d, RestartArgs a)
{
    const int m = blockIdx.x, t = threadIdx.x;
    const size_t b = (size_t)a.list[m];
    const int *cr = a.contacts + (size_t)m * (p.P + 1) * 4;
    if (t == 0) {
        d.sel[b] = sel_code(0, 0);  // nominal and working rows in buffer 0
        ElemState E{};
        E.ovr = 1;       // every knot's stored GRF values come from cf_u (zero forces)
        E.td_stale = 1;  // no touchdown value computed yet
        d.el[b] = E;
    }
    // one touchdown constraint per phase towards the next phase's contact (add_tconstr_one_phase,
    // HKDProblem.cpp:104, 268-308), none where no leg touches down; phases past the element's: none
    if (t < p.P * MTD) {
        const int i = t / MTD, j = t % MTD;
        int c[4], cn[4];
        for (int l = 0; l < 4; ++l) { c[l] = cr[i * 4 + l]; cn[l] = cr[(i + 1) * 4 + l]; }
        const int legs = td_bits(c, cn);
        d.td_mask[(b * p.P + i) * MTD + j] = (j == 0 && legs) ? legs | TD_STALE : 0;
    }
    for (int e = t; e < p.P * MTD * 4; e += 64) {
        d.al_sigma[b * p.P * MTD * 4 + e] = p.td_sigma;
        d.al_lambda[b * p.P * MTD * 4 + e] = p.td_lambda;
    }
    if (t < p.P * 4) d.term_h[b * p.P * 4 + t] = 0.0;
    for (int e = t; e < (p.P + 1) * 4; e += 64) ((int *)d.contacts)[b * (p.P + 1) * 4 + e] = cr[e];
    if (a.x0 && t < NX) ((double *)d.x0)[b * NX + t] = a.x0[(size_t)m * NX + t];
    if (a.lay) {  // the element's layout record (a per-element handle patched in place)
        constexpr int W = sizeof(Layout) / sizeof(int);
        const int *src = (const int *)(a.lay + m);
        int *dst = (int *)(d.lay + b);
        for (int e = t; e < W; e += 64) dst[e] = src[e];
    }
}

void launch_restart(const Params &p, const Bufs &d, const RestartArgs &a, hipStream_t st)
{
    if (a.n < 1) return;
    const long ns = (long)a.n * p.S * SLOT_U;
    hipLaunchKernelGGL(k_restart_slots, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, p, d, a);
    const long nk = (long)p.Kc * KCW / (p.fp32 ? 4 : 2), ne = (long)p.Kc * (p.fp32 ? KNOT_U32 : KNOT_U);
    for (int m0 = 0; m0 < a.n; m0 += 65535) {
        const dim3 g((unsigned)((nk + 255) / 256 + (ne + 255) / 256), (unsigned)(a.n - m0 < 65535 ? a.n - m0 : 65535));
        if (p.fp32) hipLaunchKernelGGL(k_restart_knots<float>, g, dim3(256), 0, st, p, d, a, d.K32, m0);
        else hipLaunchKernelGGL(k_restart_knots<double>, g, dim3(256), 0, st, p, d, a, d.K, m0);
    }
    hipLaunchKernelGGL(k_restart_elem, dim3((unsigned)a.n), dim3(64), 0, st, p, d, a);
}

}  // namespace hsddp
