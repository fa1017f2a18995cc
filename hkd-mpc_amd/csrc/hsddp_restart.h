// hsddp_restart.h — kernel interface of hsddp_restart_elements (hsddp_restart.hip).
#pragma once

#include "hsddp_internal.h"

namespace hsddp {

// The restarted elements, compacted: entry m of every array belongs to element list[m].  All
// pointers are device memory; the strides (S, P, Kc) are the handle's after the restart's layouts
// were installed.
struct RestartArgs {
    int n;                  // restarted elements
    const int *list;        // [n] element index
    const int *start;       // [n] window start sample
    const int *map_id;      // [n] row of slot_idx (one per distinct new layout)
    const int *slot_idx;    // [n_maps][S] sample offset of each state slot within the window
    const int *contacts;    // [n][P + 1][4] contact rows of the new phases (row P_b: the next contact)
    const double *x0;       // [n][24], or null: left pending
    const double *table;    // [table_n][RT_W] reference samples (hsddp_mpc.h)
    int table_n;
    const Layout *lay;      // [n] the elements' new layout records for Bufs::lay, or null: installed already
    int build_refs;         // 1: the elements' reference rows and columns are formed here (per-element
                            // references); 0: they are shared and already built, Xbar copies them
};

// every restarted element as hsddp_upload_problem + hsddp_upload_warm_start(NULL, NULL, NULL)
// leave a new problem's element; nothing of any other element is written.  n = 0 launches nothing.
void launch_restart(const Params &p, const Bufs &d, const RestartArgs &a, hipStream_t st);

}  // namespace hsddp
