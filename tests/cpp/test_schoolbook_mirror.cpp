// The reference's unit test of the schoolbook circuit (circuits/falcon_schoolbook.rs:141-169,
// test_schoolbook_verification_r1cs) re-stated on the C++ host mirror, plus its row of examples/constraint_counts.rs.
//   structure      CPU only: setup-mode counts == README.md:45,56 and frw_layout_schoolbook
//   gpu            the unit test itself: every witness value from the HIP engine (frw_witness_schoolbook_verify)
#include <cstdio>
#include <string>

#include "../../falcon-r1cs_amd/csrc/host/frw_host.hpp"

using namespace frw::host;

static int failures = 0;
#define EXPECT(cond)                                                                \
    do {                                                                            \
        if (!(cond)) { std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

// count_verify_with_schoolbook_constraints: structure only (setup mode: no values, no engine)
static void structure(int logn)
{
    const size_t N = (size_t)1 << logn;
    auto cs = ConstraintSystem::new_ref();
    cs->set_setup_mode(true);
    Polynomial z{std::vector<uint16_t>(N, 0)};
    FalconSchoolBookVerificationCircuit::build_circuit(z, z, z, logn).generate_constraints(cs);
    std::printf("Falcon-%zu |verify with schoolbook|\t%8zu |\t%8zu |\t%8zu |\n", N, cs->num_instance_variables(), cs->num_witness_variables(),
                cs->num_constraints());
    frw_layout_schoolbook_t L;
    EXPECT(frw_layout_schoolbook(logn, &L) == FRW_OK);
    EXPECT(cs->num_instance_variables() == (size_t)L.num_instance && cs->num_witness_variables() == (size_t)L.num_witness &&
           cs->num_constraints() == (size_t)L.num_constraints);
    EXPECT(cs->num_witness_variables() == (logn == 9 ? 312882u : 1150004u) && cs->num_constraints() == (logn == 9 ? 315956u : 1156150u));
}

// inner_product_mod has no stand-alone engine request: outside the circuit it reports AssignmentMissing
static void test_inner_product_mod_alone_is_assignment_missing()
{
    auto cs = ConstraintSystem::new_ref();
    std::vector<FpVar> a{FpVar::new_witness(cs, Fr::from(3))}, b{FpVar::new_witness(cs, Fr::from(5))};
    bool threw = false;
    try { inner_product_mod(cs, a, b.data(), b.size(), FpVar::new_constant(cs, Fr::from(MODULUS))); }
    catch (const SynthesisError &e) { threw = e.kind == SynthesisError::AssignmentMissing; }
    EXPECT(threw);
}

// falcon_schoolbook.rs:141-169
static void test_schoolbook_verification_r1cs(const Engine &engine, int logn)
{
    const size_t N = (size_t)1 << logn;
    Polynomial sig{std::vector<uint16_t>(N)}, pk{std::vector<uint16_t>(N)}, hm{std::vector<uint16_t>(N)};
    EXPECT(frw_synth_triples(logn, 1, 20260000 + logn, 0, sig.c.data(), pk.c.data(), hm.c.data()) == FRW_OK);   // keygen + sign_with_seed
    auto cs = ConstraintSystem::new_ref();
    cs->attach_engine(&engine);
    FalconSchoolBookVerificationCircuit::build_circuit(pk, hm, sig, logn).generate_constraints(cs);
    std::printf("number of variables %zu %zu and constraints %zu\n", cs->num_instance_variables(), cs->num_witness_variables(), cs->num_constraints());
    EXPECT(cs->is_satisfied());
    frw_layout_schoolbook_t L;
    frw_layout_schoolbook(logn, &L);
    EXPECT(cs->num_witness_variables() == (size_t)L.num_witness && cs->num_constraints() == (size_t)L.num_constraints);
    // public inputs are the coefficients themselves
    EXPECT(cs->instance_assignment[1] == Fr::from(pk.c[0]) && cs->instance_assignment[1 + N] == Fr::from(hm.c[0]));
    // a product bumped by one: the system notices
    cs->witness_assignment[29 * N + 3 * (N + 34) + 2 + 9] = cs->witness_assignment[29 * N + 3 * (N + 34) + 2 + 9] + Fr::one();
    EXPECT(!cs->is_satisfied());
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "structure";
    if (mode == "structure") {
        for (int logn : {9, 10}) structure(logn);
        test_inner_product_mod_alone_is_assignment_missing();
    } else if (mode == "gpu") {
        Engine engine(0);
        test_schoolbook_verification_r1cs(engine, 9);
        test_schoolbook_verification_r1cs(engine, 10);
    } else {
        std::printf("usage: %s structure | gpu\n", argv[0]);
        return 2;
    }
    std::printf(failures ? "%d FAILED\n" : "all passed\n", failures);
    return failures ? 1 : 0;
}
