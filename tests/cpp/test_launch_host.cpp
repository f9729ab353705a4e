// Test-only: the host side of the launchers (falcon-r1cs_amd/csrc/frw_launch.h), as a program of its own that
// tests/test_launch_host.py builds with -fsanitize=address,undefined and runs.  Nothing but the header: no device, no library.
//   Variants: for every family, every run-time tuple of a box around its values is dispatched; a tuple of the list calls the functor
//   exactly once with the same compile-time tuple, any other is reported and calls nothing.  The lists are held to the instantiations
//   written out here (the kernels' own set), and index() to a bijection from each list onto [0, size).
//   Residency: what fill() stores for a variant is what the lookup of that variant returns; an unknown variant reads 0.
//   resident_grid / verify_shape: the table of launch shapes at 256 CUs (and two small-chip cases), computed from the code before the
//   arithmetic moved into the header.
#include <stdio.h>
#include <set>
#include <utility>
#include <vector>
#include "frw_launch.h"

namespace {
int failures = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            printf("FAILED %s: ", #cond);               \
            printf(__VA_ARGS__);                        \
            printf("\n");                               \
            failures++;                                 \
        }                                               \
    } while (0)

using Tuple = std::vector<int>;

template <class Family, class F, size_t... K> bool dispatch_tuple(F &&f, const Tuple &v, std::index_sequence<K...>)
{
    return Family::dispatch(f, v[K]...);
}
template <class Family, size_t... K> int index_tuple(const Tuple &v, std::index_sequence<K...>) { return Family::index(v[K]...); }
template <class Family, size_t... K> int lookup_tuple(const frw::Residency<Family> &table, const Tuple &v, std::index_sequence<K...>)
{
    return table(v[K]...);
}

// every tuple of [lo, hi]^RANK, in order
std::vector<Tuple> box(size_t rank, int lo, int hi)
{
    std::vector<Tuple> all(1);
    for (size_t r = 0; r < rank; r++) {
        std::vector<Tuple> next;
        for (const Tuple &t : all)
            for (int v = lo; v <= hi; v++) {
                next.push_back(t);
                next.back().push_back(v);
            }
        all.swap(next);
    }
    return all;
}

int variants_checked = 0;
template <class Family, size_t RANK> void check_family(const char *name, const std::set<Tuple> &want)
{
    const auto seq = std::make_index_sequence<RANK>{};
    CHECK((size_t)Family::size == want.size(), "%s: %d variants, %zu instantiations", name, Family::size, want.size());
    // for_each: the list itself, and index() over it
    std::set<Tuple> listed;
    std::set<int> slots;
    Family::for_each([&](auto... c) {
        const Tuple t{decltype(c)::value...};
        CHECK(listed.insert(t).second, "%s: a variant is enumerated twice", name);
        const int i = Family::index(c...);
        CHECK(i >= 0 && i < Family::size, "%s: index %d outside [0, %d)", name, i, Family::size);
        CHECK(slots.insert(i).second, "%s: two variants share slot %d", name, i);
    });
    CHECK(listed == want, "%s: the list is not the kernels' set of instantiations", name);
    CHECK(slots.size() == (size_t)Family::size, "%s: %zu slots for %d variants", name, slots.size(), Family::size);
    // dispatch: every run-time tuple around the values (logn 8 and 11, enc -1 .. 4, kind 6, ... are all in the box)
    for (const Tuple &t : box(RANK, -1, 12)) {
        int calls = 0;
        Tuple got;
        const bool found = dispatch_tuple<Family>([&](auto... c) {
            calls++;
            got = Tuple{decltype(c)::value...};
        }, t, seq);
        if (want.count(t)) {
            CHECK(found && calls == 1 && got == t, "%s: a variant of the list: found %d, %d calls", name, (int)found, calls);
            variants_checked++;
        } else {
            CHECK(!found && calls == 0, "%s: a tuple outside the list: found %d, %d calls", name, (int)found, calls);
            CHECK(index_tuple<Family>(t, seq) == -1, "%s: a tuple outside the list has a slot", name);
        }
    }
    // a table: what was filled for a variant is what its lookup reads; anything else reads 0
    frw::Residency<Family> table;
    table.fill([](auto... c) { return 100 + Family::index(c...); });
    for (const Tuple &t : box(RANK, -1, 12)) {
        const int i = index_tuple<Family>(t, seq);
        const int got = lookup_tuple(table, t, seq);
        CHECK(got == (i < 0 ? 0 : 100 + i), "%s: lookup reads %d for slot %d", name, got, i);
    }
}

template <class Family, class... I> bool refused(I... v)
{
    int calls = 0;
    const bool found = Family::dispatch([&](auto...) { calls++; }, v...);
    return !found && calls == 0 && Family::index(v...) == -1;
}

struct Shape { int grid; size_t full; };
Shape shape(size_t batch, int num_cu, int occ, bool may_split)
{
    Shape s{-1, (size_t)-1};
    frw::verify_shape(batch, num_cu, occ, may_split, s.grid, s.full);
    return s;
}
}  // namespace

int main()
{
    using namespace frw;
    // the instantiations the launchers of frw_kernels.hip may reach, written out
    std::set<Tuple> ntt, expand, two, statement, modq, gadget;
    for (int logn : {9, 10}) {
        for (int enc : {0, 1, 2, 3}) ntt.insert({logn, enc});
        for (int enc : {1, 3}) expand.insert({logn, enc});
        for (int enc : {0, 1}) two.insert({logn, enc});                 // dual, schoolbook (ENC); falcon_verify (RULE)
        for (int enc : {0, 1, 3}) modq.insert({logn, enc});
        for (int form : {0, 1})
            for (int enc : {0, 1, 3}) statement.insert({logn, form, enc});
    }
    for (int kind = 0; kind < 6; kind++)
        for (int enc : {0, 1, 3}) gadget.insert({kind, enc});
    check_family<WitnessNttVariants, 2>("witness_ntt_verify", ntt);
    check_family<ExpandVariants, 2>("expand", expand);
    check_family<WitnessDualVariants, 2>("witness_dual_ntt_verify", two);
    check_family<WitnessSchoolbookVariants, 2>("witness_schoolbook_verify", two);
    check_family<StatementVariants, 3>("statement", statement);
    check_family<FalconVerifyVariants, 2>("falcon_verify", two);
    check_family<NttModqVariants, 2>("ntt_modq", modq);
    check_family<GadgetVariants, 2>("gadget", gadget);
    // the refusals by name
    CHECK((refused<WitnessNttVariants>(8, 1) && refused<WitnessNttVariants>(11, 1)), "logn 8 and 11");
    CHECK((refused<StatementVariants>(8, 0, 1) && refused<StatementVariants>(11, 1, 3)), "logn 8 and 11 of the statement");
    CHECK(refused<ExpandVariants>(10, 2), "the expansion has no ENC 2");
    CHECK((refused<WitnessDualVariants>(9, 3) && refused<WitnessSchoolbookVariants>(9, 3)), "dual and schoolbook have no ENC 3");
    CHECK(refused<FalconVerifyVariants>(9, 2), "rule 2");
    CHECK(refused<GadgetVariants>(6, 1), "gadget kind 6");

    // (batch, occ, may_split) -> (grid, full) at 256 CUs; occ 0 falls back to 2
    static const struct { size_t batch; int occ; bool split; int grid; size_t full; } table[] = {
        {1, 3, true, 5, 0},             {1, 3, false, 1, 1},             {1, 4, true, 5, 0},             {1, 0, true, 5, 0},
        {153, 3, true, 765, 0},         {153, 3, false, 153, 153},       {153, 4, true, 765, 0},         {153, 0, true, 153, 153},
        {154, 3, true, 154, 154},       {154, 3, false, 154, 154},       {154, 4, true, 770, 0},         {154, 0, true, 154, 154},
        {768, 3, true, 768, 768},       {768, 3, false, 768, 768},       {768, 4, true, 768, 768},       {768, 0, true, 384, 768},
        {769, 3, true, 768, 768},       {769, 3, false, 768, 769},       {769, 4, true, 769, 769},       {769, 0, true, 512, 512},
        {4096, 3, true, 2048, 4096},    {4096, 3, false, 2048, 4096},    {4096, 4, true, 2048, 4096},    {4096, 0, true, 2048, 4096},
        {8192, 3, true, 2048, 8192},    {8192, 3, false, 2048, 8192},    {8192, 4, true, 4096, 8192},    {8192, 0, true, 2048, 8192},
        {32768, 3, true, 3072, 30720},  {32768, 3, false, 3072, 32768},  {32768, 4, true, 4096, 32768},  {32768, 0, true, 2048, 32768},
        {100000, 3, true, 3072, 98304}, {100000, 3, false, 3072, 100000}, {100000, 4, true, 4096, 98304}, {100000, 0, true, 2048, 98304},
    };
    for (const auto &r : table) {
        const Shape s = shape(r.batch, 256, r.occ, r.split);
        CHECK(s.grid == r.grid && s.full == r.full, "verify_shape(%zu, 256, %d, %d) = (%d, %zu), not (%d, %zu)", r.batch, r.occ, (int)r.split,
              s.grid, s.full, r.grid, r.full);
    }
    // the expansion kernel's grid: resident_grid(batch, 256, 3, oversub = 8)
    static const struct { size_t batch; int grid; } expansion[] = {{1, 1}, {768, 768}, {4096, 2048}, {8192, 4096}, {32768, 4096}, {65536, 6144}};
    for (const auto &r : expansion) {
        const int g = resident_grid(r.batch, 256, 3, 8);
        CHECK(g == r.grid, "resident_grid(%zu, 256, 3, 8) = %d, not %d", r.batch, g, r.grid);
    }
    // a small chip
    CHECK(resident_grid(3072, 256, 2) == 1536, "resident_grid(3072, 256, 2) = %d", resident_grid(3072, 256, 2));
    const Shape small = shape(100, 8, 2, true);
    CHECK(small.grid == 50 && small.full == 100, "verify_shape(100, 8, 2, true) = (%d, %zu)", small.grid, small.full);

    printf("%d variants of 8 families dispatched, %zu launch shapes\n", variants_checked, sizeof table / sizeof table[0] + 6 + 2);
    if (failures) printf("launch_host: %d FAILURES\n", failures);
    else printf("launch_host: clean\n");
    return failures ? 1 : 0;
}
