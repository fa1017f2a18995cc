// element_weights_check — what the per-robot weight rows add to the host code, without HIP or a GPU
// (tests/test_element_weights_host.py):
//  * hsddp_dispatch.h: with_flags_tables for N = 0 .. 4 flags, every combination, and the four
//    (terrain table, weight table) cases — the callable runs once, its constants equal the flags in
//    argument order, and its pack after them is (), (terrain), (weights) or (terrain, weights);
//  * hsddp_phases.cpp: export_element carries a robot's row exactly while the view has rows.
// Prints "N flags calls seen terrain weights pack" per dispatch call and "export b has first last"
// per exported element; returns 1 if any line is wrong.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "hsddp_dispatch.h"
#include "hsddp_phases.h"

using hsddp::with_flags_tables;

struct Row { double v; };  // stands for the kernels' weight row type

static int failures = 0;

template <typename C>
static int bit_of(C, int at) { return (C::value ? 1 : 0) << at; }
static int bit_of(const double *, int) { return 0; }
static int bit_of(const Row *, int) { return 0; }
template <typename... A>
static int bits_of(A... a)
{
    int at = 0, v = 0;
    ((v |= bit_of(a, at++)), ...);
    return v;
}
// the pack after the constants: 0 none, 1 (terrain), 2 (weights), 3 (terrain, weights); -1 anything else
template <typename... A>
static int pack_of(int n, A...)
{
    const bool ptr[] = {std::is_pointer_v<A>..., false};
    const bool row[] = {std::is_same_v<A, const Row *>..., false};
    const int total = (int)sizeof...(A);
    for (int i = 0; i < n && i < total; ++i)
        if (ptr[i]) return -1;
    if (total == n) return 0;
    if (total == n + 1 && ptr[n]) return row[n] ? 2 : 1;
    if (total == n + 2 && ptr[n] && !row[n] && row[n + 1]) return 3;
    return -1;
}

template <typename... B>
static void check(int flags, B... b)
{
    const int n = (int)sizeof...(B);
    const double tv = 0.0;
    const Row rv{0.0};
    for (int which = 0; which < 4; ++which) {
        const double *terrain = (which & 1) ? &tv : nullptr;
        const Row *weights = (which & 2) ? &rv : nullptr;
        int calls = 0, seen = -1, pack = -2;
        const void *got_t = nullptr, *got_w = nullptr;
        with_flags_tables([&](auto... a) {
            calls += 1;
            seen = bits_of(a...);
            pack = pack_of(n, a...);
            auto note = [&](auto x) {
                if constexpr (std::is_same_v<decltype(x), const double *>) got_t = x;
                if constexpr (std::is_same_v<decltype(x), const Row *>) got_w = x;
            };
            (void)note;
            (note(a), ...);
        }, terrain, weights, b...);
        std::printf("%d %d %d %d %d %d %d\n", n, flags, calls, seen, terrain ? 1 : 0, weights ? 1 : 0, pack);
        if (calls != 1 || seen != flags || pack != which || got_t != terrain || got_w != weights) failures += 1;
    }
}

static void check_export()
{
    using namespace hsddp;
    const int B = 3;
    Layout L{};
    L.P = 2; L.S = 6; L.N[0] = L.N[1] = 2; L.s0[1] = 3; L.k0[1] = 2; L.ss[0] = L.ss[1] = 3;
    std::vector<int> reach(MAXP, 0), contacts((size_t)B * 3 * 4, 1);
    std::vector<double> rows((size_t)B * NW);
    for (size_t q = 0; q < rows.size(); ++q) rows[q] = 1.0 + (double)q;
    for (int on = 0; on < 2; ++on) {
        HorizonView v{};
        v.B = B; v.Bref = B; v.Kc = 4; v.P = 2; v.S = 6; v.S_cap = 20;
        v.shared = &L; v.reach = reach.data(); v.contacts = contacts.data();
        v.weights = on ? rows.data() : nullptr;
        for (int b = 0; b < B; ++b) {
            ElementImport e;
            export_element(v, b, e);
            std::printf("export %d %d %g %g\n", b, e.has_weights, e.weights[0], e.weights[NW - 1]);
            const bool ok = on ? (e.has_weights == 1 && e.weights[0] == rows[(size_t)b * NW] && e.weights[NW - 1] == rows[(size_t)b * NW + NW - 1])
                               : (e.has_weights == 0 && e.weights[0] == 0.0 && e.weights[NW - 1] == 0.0);
            if (!ok) failures += 1;
        }
    }
}

int main()
{
    check(0);
    for (int v = 0; v < 2; ++v) check(v, (v & 1) != 0);
    for (int v = 0; v < 4; ++v) check(v, (v & 1) != 0, (v & 2) != 0);
    for (int v = 0; v < 8; ++v) check(v, (v & 1) != 0, (v & 2) != 0, (v & 4) != 0);
    for (int v = 0; v < 16; ++v) check(v, (v & 1) != 0, (v & 2) != 0, (v & 4) != 0, (v & 8) != 0);
    check(1, 2, 0);  // integer flags as the launchers pass them: non-zero is true
    check_export();
    return failures ? 1 : 0;
}
