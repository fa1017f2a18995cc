// hsddp_elements.h — element records and the kernel interface of hsddp_copy_elements,
// hsddp_export_elements and hsddp_import_elements (hsddp_elements.hip).
#pragma once

#include <cstdint>

#include "hsddp_internal.h"

namespace hsddp {

// ---- the element record (hsddp_export_elements) ---------------------------------------------------
// One fixed-size record per element: the header (the version word, the compatibility key and the
// host bookkeeping), then the device rows packed at the capacity strides (S_cap state slots,
// HSDDP_MAX_PHASES phases), every piece 16-byte aligned, the gain rows on a 128-byte line and the
// record a whole number of lines.  Since "HEL4" the element's phase overrides (PhaseOverrides,
// hsddp_phases.h) sit in a block of whole lines between the header and the payload: the header
// keeps its size and every payload piece its distance from the record's end.
constexpr uint32_t RECORD_VERSION = 0x48454c34;  // "HEL4" (HEL1: no terrain rows; HEL2: no weight row; HEL3: no phase overrides)
constexpr int REC_HIST = 256;  // solver-info history entries a record holds

// What two handles must agree on for an element of one to continue in the other.
struct ElementKey {
    int Kc, fp32;
    int S_cap;               // (records only: it sets the record's size)
    int has_table;           // references driven from a table (hsddp_set_reference_table + _build_references)
    double dt;
    uint64_t weights, cparams;  // FNV-1a of desc.weights / desc.cparams
    uint64_t table;          // ... of the table's samples
    int ref_n, win_len;
    float ref_dt, dt_sim;
};

struct RecordHeader {
    uint32_t version, pad;
    ElementKey key;
    ElementImport host;      // hsddp_phases.h
    int reb_at_init;         // the source handle's flag
    int hist_n;              // solver-info entries held
};

// byte offsets of a record's pieces from the record's start
constexpr size_t PW_BLOCK = (sizeof(PhaseOverrides) + 127) & ~(size_t)127;

struct RecordLayout {
    size_t bytes;
    size_t pw;                           // the PhaseOverrides block (0: a layout without it)
    size_t K;                            // [Kc][KCW] reals
    size_t Xn, Xw, Dw, dX, rx, ru;       // [S_cap][24] doubles: nominal, working, Defect, dX, ref_x, ref_u
    size_t rf, d32;                      // [S_cap][12] doubles (ref_foot), [S_cap][24] floats (fp32 Defect)
    size_t scost, sfeas, sviol, sdiv;    // [S_cap]
    size_t Un, Uw, dU, du;               // [Kc][24]
    size_t rdel, reps, cfu, cff;         // [Kc][20], [Kc][20], [Kc][12], [Kc] ints
    size_t tdm, als, all, th;            // [MAXP][MTD] ints, [MAXP][MTD][4], [MAXP][MTD][4], [MAXP][4]
    size_t con, x0, el, sel, hist;       // [(MAXP + 1) * 4] ints, [24], ElemState, int, [REC_HIST][4] floats
};

// overrides: with the PhaseOverrides block, as every record the library writes or reads has it;
// without: the header and the payload alone, the offsets the block then shifts by PW_BLOCK
inline RecordLayout record_layout(int Kc, size_t S_cap, int fp32, bool overrides = false)
{
    RecordLayout R{};
    size_t at = (sizeof(RecordHeader) + 127) & ~(size_t)127;
    if (overrides) { R.pw = at; at += PW_BLOCK; }
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 15) & ~(size_t)15; return o; };
    R.K = take((size_t)Kc * KCW * (fp32 ? 4 : 8));
    const size_t row = NX * sizeof(double);
    R.Xn = take(S_cap * row); R.Xw = take(S_cap * row); R.Dw = take(S_cap * row); R.dX = take(S_cap * row);
    R.rx = take(S_cap * row); R.ru = take(S_cap * row);
    R.rf = take(S_cap * 12 * sizeof(double));
    R.d32 = take(fp32 ? S_cap * NX * sizeof(float) : 0);
    R.scost = take(S_cap * 8); R.sfeas = take(S_cap * 8); R.sviol = take(S_cap * 8); R.sdiv = take(S_cap * 4);
    R.Un = take(Kc * row); R.Uw = take(Kc * row); R.dU = take(Kc * row); R.du = take(Kc * row);
    R.rdel = take((size_t)Kc * 20 * 8); R.reps = take((size_t)Kc * 20 * 8);
    R.cfu = take((size_t)Kc * 12 * 8); R.cff = take((size_t)Kc * 4);
    R.tdm = take(MAXP * MTD * 4); R.als = take(MAXP * MTD * 4 * 8); R.all = take(MAXP * MTD * 4 * 8);
    R.th = take(MAXP * 4 * 8);
    R.con = take((MAXP + 1) * 4 * 4); R.x0 = take(row); R.el = take(sizeof(ElemState)); R.sel = take(4);
    R.hist = take((size_t)REC_HIST * 4 * sizeof(float));
    R.bytes = (at + 127) & ~(size_t)127;
    return R;
}

// ---- the kernels ------------------------------------------------------------------------------------
// One side of a move: a handle's buffers at that handle's strides, or packed records.
struct ElemSide {
    Bufs d;            // the handle's buffers (rec null)
    char *rec;         // records' base, RecordLayout::bytes apart (null: the handle)
    const int *idx;    // [n] the element (or record) of move m; null: m itself
    int P, S;          // strides of the per-phase and per-slot rows (records: MAXP, S_cap)
    int hcap;          // solver-info entries per element
    int shared_refs;   // the handle holds one reference row set for the batch
};

struct MoveArgs {
    int n;                   // moves
    int Kc, fp32;
    RecordLayout R;
    const Layout *lay;       // [n] the destination's layout records for Bufs::lay, or null: installed already
};

// Move m copies element src.idx[m] of the source side to element dst.idx[m] of the destination side:
// the nominal and working rows read through the source's sel (untouched) and written to buffers 0
// and 1 (0 alone where they coincide), the gains, the search direction, the references with their
// entry-major columns, the constraint parameters and stored values, ElemState, the solver-info
// rows held, the slot sums, x0 and the contact rows.  Nothing of any other element is written;
// n = 0 launches nothing.  No element may be both read and written by one launch.
void launch_move(const MoveArgs &a, const ElemSide &src, const ElemSide &dst, hipStream_t st);

}  // namespace hsddp
