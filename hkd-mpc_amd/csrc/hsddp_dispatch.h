// hsddp_dispatch.h — the host side of a kernel launch: runtime flags to template arguments.
// Plain C++17 without a HIP include (tests/drivers/dispatch_check.cpp compiles it with g++).
//
// A launcher names its kernel and its argument list once:
//     with_flags([&](auto el, auto wide) {
//         hipLaunchKernelGGL((k<decltype(el)::value, decltype(wide)::value>), grid, block, 0, st, p, d);
//     }, p.elem_layout, p.S >= RW);
// Axes that are not free booleans (the sweep's precision and waves per block) stay explicit branches
// around it, so no instantiation exists that the branches do not reach.
#pragma once
#include <type_traits>

namespace hsddp {

// f(std::bool_constant<flag>{}...) for the runtime flags, in argument order; f is called exactly once
template <bool... Known, typename F>
void with_flags(F &&f)
{
    f(std::bool_constant<Known>{}...);
}
template <bool... Known, typename F, typename... Rest>
void with_flags(F &&f, bool b, Rest... rest)
{
    if (b) with_flags<Known..., true>(f, rest...);
    else with_flags<Known..., false>(f, rest...);
}

// ... and with the table as f's last argument while it is non-null, else without it: the kernels that
// read the terrain end in an argument pack (TerrT, hsddp_device.h) that holds the handle's table or
// nothing, and f ends in `auto... tr` to pass it on
template <typename F, typename T, typename... Flags>
void with_flags_table(F &&f, const T *table, Flags... flags)
{
    if (table) with_flags([&](auto... c) { f(c..., table); }, flags...);
    else with_flags(f, flags...);
}

// ... and with a second table after the first while it is non-null (the per-robot weight rows after
// the terrain): f's pack is then (), (table), (second) or (table, second)
template <typename F, typename T, typename W, typename... Flags>
void with_flags_tables(F &&f, const T *table, const W *second, Flags... flags)
{
    if (second) with_flags_table([&](auto... c) { f(c..., second); }, table, flags...);
    else with_flags_table(f, table, flags...);
}

// ... and with the weights a handle reads (a WtsTab, hsddp_internal.h: `phase` while a phase has an
// override, else `robot` while the per-robot table is on, else neither) as that last table
template <typename F, typename WT, typename... Flags>
auto with_flags_table(F &&f, WT w, Flags... flags) -> decltype((void)w.phase)
{
    if (w.phase) with_flags_table(f, w.phase, flags...);
    else with_flags_table(f, w.robot, flags...);
}
template <typename F, typename T, typename WT, typename... Flags>
auto with_flags_tables(F &&f, const T *table, WT w, Flags... flags) -> decltype((void)w.phase)
{
    if (w.phase) with_flags_tables(f, table, w.phase, flags...);
    else with_flags_tables(f, table, w.robot, flags...);
}

static inline unsigned blocks_for(long n, int bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace hsddp
