// dispatch_check — the launchers' flag dispatch (hkd-mpc_amd/csrc/hsddp_dispatch.h) on its own,
// without HIP or a GPU (tests/test_dispatch_host.py).  For N = 0 .. 4 runtime flags and each of the
// 2^N combinations: the callable runs exactly once and its constants equal the flags in argument
// order; with_flags_table passes the table after the constants exactly when it is non-null.
// Prints one line per call, "N flags calls seen table at" (flags and seen as bits, first argument
// lowest; at: the table's argument position or -1), and returns 1 if any line is wrong.
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "hsddp_dispatch.h"

using hsddp::with_flags;
using hsddp::with_flags_table;

static int failures = 0;

template <typename C>
static int bit_of(C, int at)
{
    static_assert(std::is_same_v<C, std::bool_constant<C::value>>, "a std::bool_constant");
    return (C::value ? 1 : 0) << at;
}
static int bit_of(const double *, int) { return 0; }
template <typename... A>
static int bits_of(A... a)
{
    int at = 0, v = 0;
    ((v |= bit_of(a, at++)), ...);
    return v;
}
template <typename... A>
static int table_at(A...)
{
    int at = 0, pos = -1;
    ((std::is_pointer_v<A> ? (pos = at++) : at++), ...);
    return pos;
}

static void report(int n, int flags, int calls, int seen, bool table, int at)
{
    std::printf("%d %d %d %d %d %d\n", n, flags, calls, seen, table ? 1 : 0, at);
    if (calls != 1 || seen != flags || at != (table ? n : -1)) failures += 1;
}

template <typename... B>
static void check(int flags, B... b)
{
    const int n = (int)sizeof...(B);
    int calls = 0, seen = -1;
    with_flags([&](auto... c) {
        static_assert(sizeof...(c) == sizeof...(B), "one constant per flag");
        calls += 1;
        seen = bits_of(c...);
    }, b...);
    report(n, flags, calls, seen, false, -1);
    const double value = 0.0;
    for (const double *table : {(const double *)nullptr, &value}) {
        int at = -2;
        calls = 0;
        seen = -1;
        with_flags_table([&](auto... a) {
            calls += 1;
            seen = bits_of(a...);
            at = table_at(a...);
            if (at >= 0 && (int)sizeof...(a) != n + 1) at = -2;  // nothing after the table
        }, table, b...);
        report(n, flags, calls, seen, table != nullptr, at);
    }
}

int main()
{
    check(0);
    for (int v = 0; v < 2; ++v) check(v, (v & 1) != 0);
    for (int v = 0; v < 4; ++v) check(v, (v & 1) != 0, (v & 2) != 0);
    for (int v = 0; v < 8; ++v) check(v, (v & 1) != 0, (v & 2) != 0, (v & 4) != 0);
    for (int v = 0; v < 16; ++v) check(v, (v & 1) != 0, (v & 2) != 0, (v & 4) != 0, (v & 8) != 0);
    // integer flags as the launchers pass them (Params::fp32, ::elem_layout are ints): non-zero is true
    check(1, 2, 0);
    check(2, 0, -1);
    return failures ? 1 : 0;
}
