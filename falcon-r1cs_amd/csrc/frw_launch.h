// frw_launch.h -- how the launchers of frw_kernels.hip get from run-time arguments to a kernel instantiation, its residency and its grid.
// The persistent kernels are templates over a small closed set of compile-time variants (LOGN, ENC, FORM, RULE, KIND).  A family's
// variants are written down ONCE, as a Variants<...> list; the launch (dispatch), the residency query at context creation (for_each)
// and the residency table's slot (index) all come from that one list, so a variant that can be launched is a variant whose residency was
// asked.  Host code only, plain C++17, nothing of the HIP runtime: tests/cpp/test_launch_host.cpp holds it to its table under the sanitizers.
#pragma once
#include <stddef.h>
#include <algorithm>
#include <type_traits>

namespace frw {

// ---- variants ---------------------------------------------------------------------------------------------------------------------------
// the admissible values of one template parameter
template <int... V> struct Values {
    static constexpr int count = sizeof...(V);
    // where v stands in the list; -1: not in it
    static constexpr int find(int v)
    {
        int at = -1, i = 0;
        ((at = v == V ? i : at, i++), ...);
        return at;
    }
    // g(integral_constant<V>) for the V equal to v, and what it returns; false (g not called): no such value
    template <class G> static bool select(int v, G &&g) { return ((v == V && g(std::integral_constant<int, V>{})) || ...); }
    template <class G> static void each(G &&g) { (g(std::integral_constant<int, V>{}), ...); }
};

// a family's variants: every combination of its parameters' values, one Values<...> per parameter
template <class... Lists> struct Variants;
template <> struct Variants<> {
    static constexpr int size = 1;
    static constexpr int index() { return 0; }
    template <class F> static bool dispatch(F &&f) { f(); return true; }
    template <class F> static void for_each(F &&f) { f(); }
};
template <class L0, class... Ls> struct Variants<L0, Ls...> {
    using Rest = Variants<Ls...>;
    static constexpr int size = L0::count * Rest::size;
    // THE slot of a variant in a table of `size` entries (row-major over the lists' positions); -1: no such variant
    template <class... I> static constexpr int index(int v0, I... vs)
    {
        static_assert(sizeof...(I) == sizeof...(Ls), "one value per parameter");
        const int a = L0::find(v0), b = Rest::index(vs...);
        return a < 0 || b < 0 ? -1 : a * Rest::size + b;
    }
    // f(integral_constant...) for the variant equal to the run-time (v0, vs...); false, and f is not called: no such variant
    template <class F, class... I> static bool dispatch(F &&f, int v0, I... vs)
    {
        static_assert(sizeof...(I) == sizeof...(Ls), "one value per parameter");
        return L0::select(v0, [&](auto c0) { return Rest::dispatch([&](auto... cs) { f(c0, cs...); }, vs...); });
    }
    // f(integral_constant...) for every variant
    template <class F> static void for_each(F &&f)
    {
        L0::each([&](auto c0) { Rest::for_each([&](auto... cs) { f(c0, cs...); }); });
    }
};

// The families of frw_kernels.hip, which adds to each the instantiation that belongs to a variant.  ENC: 0 canonical, 1 Montgomery,
// 2 the compact record, 3 Montgomery form over a field registered on the context.
using LogN = Values<9, 10>;
using WitnessNttVariants = Variants<LogN, Values<0, 1, 2, 3>>;                    // LOGN, ENC
using ExpandVariants = Variants<LogN, Values<1, 3>>;                              // LOGN, ENC
using WitnessDualVariants = Variants<LogN, Values<0, 1>>;                         // LOGN, ENC
using WitnessSchoolbookVariants = Variants<LogN, Values<0, 1>>;                   // LOGN, ENC
using StatementVariants = Variants<LogN, Values<0, 1>, Values<0, 1, 3>>;          // LOGN, FORM, ENC
using FalconVerifyVariants = Variants<LogN, Values<0, 1>>;                        // LOGN, RULE
using NttModqVariants = Variants<LogN, Values<0, 1, 3>>;                          // LOGN, ENC
using GadgetVariants = Variants<Values<0, 1, 2, 3, 4, 5>, Values<0, 1, 3>>;       // KIND (G_* of frw_device.h), ENC

// Resident workgroups per CU of every variant of one family.  Filled once (before any launch; a launch may be inside a stream capture,
// where the runtime cannot be asked), read-only afterwards.  0 = never asked or no such variant: resident_grid falls back to 2.
template <class Family> struct Residency {
    int per_cu[Family::size] = {};
    // query(integral_constant...) -> resident workgroups per CU of that variant
    template <class Q> void fill(Q &&query)
    {
        Family::for_each([&](auto... c) { per_cu[Family::index(c...)] = query(c...); });
    }
    template <class... I> int operator()(I... v) const
    {
        const int i = Family::index(v...);
        return i < 0 ? 0 : per_cu[i];
    }
};

// ---- grids ------------------------------------------------------------------------------------------------------------------------------
// work items a split signature of witness_ntt_verify_kernel is cut into (frw_kernels.hip, "work distribution")
constexpr int PARTS = 5;

// Workgroups to launch for `batch` items.  `cap` = what the device keeps resident (per_cu x CUs).  Launches with at least
// two items per workgroup to spare use up to OVERSUB x cap: with more workgroups than the device holds, the ones that
// finish are replaced at different moments, which keeps the workgroups' compute and store phases from lining up across
// the chip (measured, tools/ab_variants.py: 32,768 Falcon-1024 signatures +1.3 ... 3.5 % at 2 x ... 4 x the resident 768,
// no more at 6 x and 8 x; 8,192 Falcon-512 signatures +2.7 % at 2,048 and +4.4 % at 4,096 workgroups over 1,024, -9 % at
// one signature per workgroup; the expansion kernel, whose items are all stores behind a few loads, +4.5 % at 8 x:
// profiles/r02_scheduling_ab.txt).
#ifndef FRW_OVERSUB
#define FRW_OVERSUB 4
#endif
inline int resident_grid(size_t batch, int num_cu, int per_cu, int oversub = FRW_OVERSUB)
{
    const size_t cap = (size_t)(per_cu > 0 ? per_cu : 2) * (size_t)num_cu;
    if (batch <= cap) return (int)batch;
#if defined(FRW_FORCE_GRID)          // A/B builds only
    return FRW_FORCE_GRID;
#endif
    // beyond the resident capacity only while every workgroup keeps at least two items
    size_t top = cap;
    if (batch >= 2 * cap) top = std::min((size_t)oversub * cap, batch / 2);
    // Every workgroup streams one 2.5-5 MB signature at a time, so a batch that is not a multiple of the grid ends in a
    // tail where most CUs idle.  For short launches (< 8 rounds) a grid between 5/8 and 8/8 of the target that divides the
    // batch wins (4,096 signatures: 512 x 8 rounds beats 768 x 5.33 by 1.1 %); long launches amortise the tail, and the
    // witness kernel splits it besides.
    if (batch < 8 * top)
        for (size_t g = top; g * 8 >= top * 5; g--)
            if (batch % g == 0) return (int)g;
    return (int)top;
}

// (grid, full) of a witness launch: all-split for small batches, one workgroup per signature up to the resident capacity,
// else the resident grid (or, for short launches, a divisor of the batch close to it) with the ragged tail split.
inline void verify_shape(size_t batch, int num_cu, int occ, bool may_split, int &grid, size_t &full)
{
    const size_t cap = (size_t)(occ > 0 ? occ : 2) * (size_t)num_cu;
    if (may_split && batch * PARTS <= cap) {     // measured: 1 signature 167 -> 56 us, 64 signatures 172 -> 95 us; at 256 it loses
        grid = (int)(batch * PARTS);
        full = 0;
        return;
    }
    grid = resident_grid(batch, num_cu, occ);
    full = may_split ? batch / (size_t)grid * (size_t)grid : batch;
}

}  // namespace frw
