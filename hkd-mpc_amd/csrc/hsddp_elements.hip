// hsddp_elements.hip — elements moved between slots, handles and host records
// (hsddp_copy_elements, hsddp_export_elements, hsddp_import_elements): everything a robot carries
// from one MPC tick to the next, copied so that the robot cannot tell.
//
// The moves come as a compacted list and every kernel's grid is (work of one element) x (listed
// moves): the cost follows the number of moved elements, not B.  Either side of a move is a handle's
// buffers at that handle's strides or a packed record (ElemSide, hsddp_elements.h), so one kernel
// family serves handle -> handle (copy), handle -> record (export, and the staging of a same-handle
// move's overlapping sources) and record -> handle (import):
//
//   k_move_slots   per state slot: Xbar, X, Defect, dX, the reference rows (and the destination's
//                  entry-major columns), the fp32 Defect copy, the slot sums
//   k_move_knots   per control slot: the compact gain rows (one contiguous run of whole 128-byte
//                  lines per element), Ubar, U, dU, du, the ReB pair of every GRF row, the stored
//                  GRF forces and their flag
//   k_move_elem    per element: buffer selector, ElemState, the solver-info rows held, the touchdown
//                  slots of every phase with their AL parameters and stored values, the contact
//                  rows, x0, the layout record
//
// The source's nominal and working rows are read through its sel and land in buffers 0 and 1 of the
// destination (buffer 0 alone where the two coincide); the source is only read.  The row loads and
// stores are 16 bytes wide and consecutive lanes take consecutive pieces of a row, as
// hsddp_restart.hip's do.
#include "hsddp_device.h"
#include "hsddp_elements.h"

namespace hsddp {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

namespace {

DEV size_t elem_of(const ElemSide &a, int m) { return a.idx ? (size_t)a.idx[m] : (size_t)m; }

// the side's selector code of element e
DEV int sel_of(const ElemSide &a, const RecordLayout &R, size_t e)
{
    return a.rec ? *(const int *)(a.rec + e * R.bytes + R.sel) : a.d.sel[e];
}

// state-slot rows
enum { XN, XW, DW, DX, RX, RU, RF, D32, SCOST, SFEAS, SVIOL, SDIV };
// row s of element e (nb, wb: the nominal and working buffers of a handle side)
DEV char *slot_row(const ElemSide &a, const RecordLayout &R, int w, size_t e, int s, int nb, int wb)
{
    if (a.rec) {
        char *r = a.rec + e * R.bytes;
        switch (w) {
        case XN: return r + R.Xn + (size_t)s * 192;
        case XW: return r + R.Xw + (size_t)s * 192;
        case DW: return r + R.Dw + (size_t)s * 192;
        case DX: return r + R.dX + (size_t)s * 192;
        case RX: return r + R.rx + (size_t)s * 192;
        case RU: return r + R.ru + (size_t)s * 192;
        case RF: return r + R.rf + (size_t)s * 96;
        case D32: return r + R.d32 + (size_t)s * 96;
        case SCOST: return r + R.scost + (size_t)s * 8;
        case SFEAS: return r + R.sfeas + (size_t)s * 8;
        case SVIOL: return r + R.sviol + (size_t)s * 8;
        default: return r + R.sdiv + (size_t)s * 4;
        }
    }
    const size_t row = e * a.S + s, rr = (a.shared_refs ? 0 : e) * a.S + s;
    switch (w) {
    case XN: return (char *)(xbuf(a.d, nb) + row * NX);
    case XW: return (char *)(xbuf(a.d, wb) + row * NX);
    case DW: return (char *)(dbuf(a.d, wb) + row * NX);
    case DX: return (char *)(a.d.dX + row * NX);
    case RX: return (char *)(a.d.ref_x + rr * NX);
    case RU: return (char *)(a.d.ref_u + rr * NX);
    case RF: return (char *)(a.d.ref_foot + rr * 12);
    case D32: return (char *)(a.d.def32 + row * NX);
    case SCOST: return (char *)(a.d.slot_cost + row);
    case SFEAS: return (char *)(a.d.slot_feas + row);
    case SVIOL: return (char *)(a.d.slot_viol + row);
    default: return (char *)(a.d.slot_div + row);
    }
}

// control-slot rows
enum { UN, UW, DU, DUU, RDEL, REPS, CFU, CFF };
DEV char *knot_row(const ElemSide &a, const RecordLayout &R, int Kc, int w, size_t e, int kc, int nb, int wb)
{
    if (a.rec) {
        char *r = a.rec + e * R.bytes;
        switch (w) {
        case UN: return r + R.Un + (size_t)kc * 192;
        case UW: return r + R.Uw + (size_t)kc * 192;
        case DU: return r + R.dU + (size_t)kc * 192;
        case DUU: return r + R.du + (size_t)kc * 192;
        case RDEL: return r + R.rdel + (size_t)kc * 160;
        case REPS: return r + R.reps + (size_t)kc * 160;
        case CFU: return r + R.cfu + (size_t)kc * 96;
        default: return r + R.cff + (size_t)kc * 4;
        }
    }
    const size_t q = e * Kc + kc;
    switch (w) {
    case UN: return (char *)(ubuf(a.d, nb) + q * NU);
    case UW: return (char *)(ubuf(a.d, wb) + q * NU);
    case DU: return (char *)(a.d.dU + q * NU);
    case DUU: return (char *)(a.d.du + q * NU);
    case RDEL: return (char *)(a.d.reb_delta + q * 20);
    case REPS: return (char *)(a.d.reb_eps + q * 20);
    case CFU: return (char *)(a.d.cf_u + q * 12);
    default: return (char *)(a.d.cf_flag + q);
    }
}

// per-phase and per-element rows
enum { TDM, ALS, ALL, TH, CON, X0, EL, HIST };
DEV char *elem_row(const ElemSide &a, const RecordLayout &R, int w, size_t e)
{
    if (a.rec) {
        char *r = a.rec + e * R.bytes;
        switch (w) {
        case TDM: return r + R.tdm;
        case ALS: return r + R.als;
        case ALL: return r + R.all;
        case TH: return r + R.th;
        case CON: return r + R.con;
        case X0: return r + R.x0;
        case EL: return r + R.el;
        default: return r + R.hist;
        }
    }
    switch (w) {
    case TDM: return (char *)(a.d.td_mask + e * a.P * MTD);
    case ALS: return (char *)(a.d.al_sigma + e * a.P * MTD * 4);
    case ALL: return (char *)(a.d.al_lambda + e * a.P * MTD * 4);
    case TH: return (char *)(a.d.term_h + e * a.P * 4);
    case CON: return (char *)((int *)a.d.contacts + e * (a.P + 1) * 4);
    case X0: return (char *)((double *)a.d.x0 + e * NX);
    case EL: return (char *)(a.d.el + e);
    default: return (char *)(a.d.hist + e * a.hcap * 4);
    }
}

DEV char *gain_rows(const ElemSide &a, const RecordLayout &R, const MoveArgs &g, size_t e)
{
    if (a.rec) return a.rec + e * R.bytes + R.K;
    const size_t bytes = (size_t)g.Kc * KCW * (g.fp32 ? 4 : 8);
    return (g.fp32 ? (char *)a.d.K32 : (char *)a.d.K) + e * bytes;
}

// the destination's buffers: the nominal rows in 0, the working rows in 1 unless they are the nominal's
DEV int dst_work(int sel) { return (sel & 3) == ((sel >> 2) & 3) ? 0 : 1; }

}  // namespace

// 16-byte pieces of one state slot: Xbar, X, Defect, dX, ref_x, ref_u 12 each, ref_foot 6, the slot
// sums 1; the fp32 Defect copy 6 more
constexpr int MSLOT_U = 6 * (NX / 2) + 6 + 1, MSLOT_U32 = MSLOT_U + 6;

// One thread per (move, state slot, piece); rows: the slots both sides hold (an element's own slots
// lie within either stride).
__global__ __launch_bounds__(256) void k_move_slots(MoveArgs g, ElemSide src, ElemSide dst, int rows)
{
    const int SU = g.fp32 ? MSLOT_U32 : MSLOT_U;
    const long per = (long)rows * SU, gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)g.n * per) return;
    const int m = (int)(gid / per), s = (int)(gid % per / SU);
    int u = (int)(gid % SU);
    const size_t es = elem_of(src, m), ed = elem_of(dst, m);
    const int sel = sel_of(src, g.R, es), nb = sel & 3, wb = (sel >> 2) & 3, dw = dst_work(sel);
    const int w = u / (NX / 2);
    if (w < 6) {  // one of the six 24-wide rows
        u -= w * (NX / 2);
        if (w == XW && dw == 0 && !dst.rec) return;  // (the nominal rows are the working rows)
        const d2 v = ((const d2 *)slot_row(src, g.R, w, es, s, nb, wb))[u];
        ((d2 *)slot_row(dst, g.R, w, ed, s, 0, dw))[u] = v;
        if ((w == RX || w == RU) && !dst.rec)  // the entry-major column pair
            ((d2 *)dst.d.ref_t)[(size_t)((w == RX ? 0 : NX / 2) + u) * dst.d.ref_tw + ed * dst.S + s] = v;
        return;
    }
    u -= 6 * (NX / 2);
    if (u < 6) {
        const d2 v = ((const d2 *)slot_row(src, g.R, RF, es, s, nb, wb))[u];
        ((d2 *)slot_row(dst, g.R, RF, ed, s, 0, dw))[u] = v;
        if (!dst.rec) ((d2 *)dst.d.ref_t)[(size_t)(NX + u) * dst.d.ref_tw + ed * dst.S + s] = v;
        return;
    }
    u -= 6;
    if (u == 0) {  // the slot's partial sums
        *(double *)slot_row(dst, g.R, SCOST, ed, s, 0, dw) = *(const double *)slot_row(src, g.R, SCOST, es, s, nb, wb);
        *(double *)slot_row(dst, g.R, SFEAS, ed, s, 0, dw) = *(const double *)slot_row(src, g.R, SFEAS, es, s, nb, wb);
        *(double *)slot_row(dst, g.R, SVIOL, ed, s, 0, dw) = *(const double *)slot_row(src, g.R, SVIOL, es, s, nb, wb);
        *(int *)slot_row(dst, g.R, SDIV, ed, s, 0, dw) = *(const int *)slot_row(src, g.R, SDIV, es, s, nb, wb);
        return;
    }
    u -= 1;  // (fp32 handles only)
    ((f4 *)slot_row(dst, g.R, D32, ed, s, 0, dw))[u] = ((const f4 *)slot_row(src, g.R, D32, es, s, nb, wb))[u];
}

// 16-byte pieces of one control slot beside its gain rows: Ubar, U, dU, du 12 each, the ReB delta
// and eps rows 10 each, the stored forces 6 (the first of them takes the flag along)
constexpr int MKNOT_U = 4 * (NU / 2) + 2 * 10 + 6;

// m0 + blockIdx.y: the move (the grid's y extent holds 65535).  The first threads of an element's x
// range copy its compact gain rows piece by piece — one contiguous run of Kc x 18 (fp32: 9) whole
// lines, every wave moving eight whole lines — the others take one piece each of the control
// slots' other rows.
__global__ __launch_bounds__(256) void k_move_knots(MoveArgs g, ElemSide src, ElemSide dst, int m0)
{
    const long nk = (long)g.Kc * KCW / (g.fp32 ? 4 : 2), t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = m0 + blockIdx.y;
    const size_t es = elem_of(src, m), ed = elem_of(dst, m);
    if (t < nk) {
        ((f4 *)gain_rows(dst, g.R, g, ed))[t] = ((const f4 *)gain_rows(src, g.R, g, es))[t];
        return;
    }
    const long e = t - (nk + 255) / 256 * 256;  // (the gain rows' last block is theirs alone)
    if (e < 0 || e >= (long)g.Kc * MKNOT_U) return;
    const int kc = (int)(e / MKNOT_U);
    int u = (int)(e % MKNOT_U);
    const int sel = sel_of(src, g.R, es), nb = sel & 3, wb = (sel >> 2) & 3, dw = dst_work(sel);
    int w = u / (NU / 2);
    if (w < 4) {
        u -= w * (NU / 2);
        if (w == UW && dw == 0 && !dst.rec) return;
    } else {
        u -= 4 * (NU / 2);
        w = u < 10 ? RDEL : u < 20 ? REPS : CFU;
        u -= w == RDEL ? 0 : w == REPS ? 10 : 20;
    }
    ((d2 *)knot_row(dst, g.R, g.Kc, w, ed, kc, 0, dw))[u] = ((const d2 *)knot_row(src, g.R, g.Kc, w, es, kc, nb, wb))[u];
    if (w == CFU && u == 0)
        *(int *)knot_row(dst, g.R, g.Kc, CFF, ed, kc, 0, dw) = *(const int *)knot_row(src, g.R, g.Kc, CFF, es, kc, nb, wb);
}

// One wave per move.  Phases past the source's stride have no touchdown slot and zero contact rows.
__global__ __launch_bounds__(64) void k_move_elem(MoveArgs g, ElemSide src, ElemSide dst)
{
    const int m = blockIdx.x, t = threadIdx.x;
    const size_t es = elem_of(src, m), ed = elem_of(dst, m);
    const int sel = sel_of(src, g.R, es);
    if (t == 0) {
        const int code = sel_code(0, dst_work(sel));
        if (dst.rec) *(int *)(dst.rec + ed * g.R.bytes + g.R.sel) = code;
        else dst.d.sel[ed] = code;
    }
    const int *Es = (const int *)elem_row(src, g.R, EL, es);
    if (t < (int)(sizeof(ElemState) / sizeof(int))) ((int *)elem_row(dst, g.R, EL, ed))[t] = Es[t];
    // the solver-info rows held (the host made room for them)
    int hn = ((const ElemState *)Es)->hist_n;
    hn = hn < src.hcap ? hn : src.hcap;
    hn = hn < dst.hcap ? hn : dst.hcap;
    const f4 *hs = (const f4 *)elem_row(src, g.R, HIST, es);
    f4 *hd = (f4 *)elem_row(dst, g.R, HIST, ed);
    for (int e = t; e < hn; e += 64) hd[e] = hs[e];
    const int Ps = src.P, Pd = dst.P;
    if (t < Pd * MTD) {
        const int i = t / MTD, j = t % MTD;
        ((int *)elem_row(dst, g.R, TDM, ed))[t] = i < Ps ? ((const int *)elem_row(src, g.R, TDM, es))[i * MTD + j] : 0;
    }
    for (int e = t; e < Pd * MTD * 4; e += 64)
        if (e / (MTD * 4) < Ps) {
            ((double *)elem_row(dst, g.R, ALS, ed))[e] = ((const double *)elem_row(src, g.R, ALS, es))[e];
            ((double *)elem_row(dst, g.R, ALL, ed))[e] = ((const double *)elem_row(src, g.R, ALL, es))[e];
        }
    if (t < Pd * 4) ((double *)elem_row(dst, g.R, TH, ed))[t] = t / 4 < Ps ? ((const double *)elem_row(src, g.R, TH, es))[t] : 0.0;
    for (int e = t; e < (Pd + 1) * 4; e += 64)
        ((int *)elem_row(dst, g.R, CON, ed))[e] = e / 4 <= Ps ? ((const int *)elem_row(src, g.R, CON, es))[e] : 0;
    if (t < NX) ((double *)elem_row(dst, g.R, X0, ed))[t] = ((const double *)elem_row(src, g.R, X0, es))[t];
    if (g.lay && !dst.rec) {  // the element's layout record (a per-element handle patched in place)
        constexpr int W = sizeof(Layout) / sizeof(int);
        const int *ls = (const int *)(g.lay + m);
        int *ld = (int *)(dst.d.lay + ed);
        for (int e = t; e < W; e += 64) ld[e] = ls[e];
    }
}

void launch_move(const MoveArgs &a, const ElemSide &src, const ElemSide &dst, hipStream_t st)
{
    if (a.n < 1) return;
    const int rows = src.S < dst.S ? src.S : dst.S;
    const long ns = (long)a.n * rows * (a.fp32 ? MSLOT_U32 : MSLOT_U);
    hipLaunchKernelGGL(k_move_slots, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, a, src, dst, rows);
    const long nk = (long)a.Kc * KCW / (a.fp32 ? 4 : 2), ne = (long)a.Kc * MKNOT_U;
    for (int m0 = 0; m0 < a.n; m0 += 65535) {
        const dim3 g((unsigned)((nk + 255) / 256 + (ne + 255) / 256), (unsigned)(a.n - m0 < 65535 ? a.n - m0 : 65535));
        hipLaunchKernelGGL(k_move_knots, g, dim3(256), 0, st, a, src, dst, m0);
    }
    hipLaunchKernelGGL(k_move_elem, dim3((unsigned)a.n), dim3(64), 0, st, a, src, dst);
}

}  // namespace hsddp
