// frw_verify.h -- what the host verifier (frw_verify.cpp) and the device's prepare_inputs (frw_verify_dev.hip) share: the prepared
// verifying key and the part of a verification that follows prepare_inputs, so that frw_groth16_verify and frw_groth16_verify_dev
// give the same verdicts by construction.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/frw.h"
#include "frw_pairing.h"

struct frw_groth16_vk {
    size_t num_instance;
    std::vector<frw::G1Affine29> gamma_abc;
    frw::pairing::G2 gamma_neg, delta_neg;
    frw::pairing::Fp12 alpha_beta;          // final_exponentiation(miller_loop(alpha_g1, beta_g2))
    frw::pairing::FrobeniusConstants fc;
    int device = -1;                        // frw_groth16_vk_load_dev: the device `msm` lives on (-1: a host key)
    frw_msm *msm = nullptr;                 // ... and gamma_abc_g1 there, as a narrow MSM handle (frw_verify_dev.hip says which kind)
    uint32_t *d_pairing = nullptr;          // ... and the device pairing's fixed part there (frw_pairing_dev.hip: line tables, constants)
    unsigned pairing_inf = 0;               // ... bit j: the fixed G2 point j (-gamma, -delta, beta) is the point at infinity
    uint64_t delta_ark[24] = {};            // delta_g2 as the key gave it (ark-ff's limbs): what frw_groth16_rerandomize adds multiples of
    uint64_t *d_delta = nullptr;            // frw_groth16_vk_load_dev: ... and the same 24 words on the device (frw_rerand.hip)
    ~frw_groth16_vk()
    {
        if (msm) frw_msm_free(msm);
        if (d_pairing) (void)hipFree(d_pairing);
        if (d_delta) (void)hipFree(d_delta);
    }
};

namespace frw {
namespace verify {

// The checks ark's deserialiser makes of a G1 point, host and device alike (the key's gamma_abc_g1 rows are checked by one or the
// other, and must be refused by both or by neither).  Raw limbs must be below the modulus BEFORE any arithmetic reduces them
// silently (x and x + q would otherwise be one point with two encodings).
__host__ __device__ inline bool fq_limbs_below_modulus(const uint64_t *w)
{
    constexpr uint64_t Q[6] = {0xb9feffffffffaaabULL, 0x1eabfffeb153ffffULL, 0x6730d2a0f6b0f624ULL,
                               0x64774b84f38512bfULL, 0x4b1ba7b6434bacd7ULL, 0x1a0111ea397fe69aULL};
    for (int k = 5; k >= 0; k--) {
        if (w[k] < Q[k]) return true;
        if (w[k] > Q[k]) return false;
    }
    return false;
}
__host__ __device__ inline bool coordinates_canonical(const uint64_t *w, int coordinates)
{
    for (int k = 0; k < coordinates; k++)
        if (!fq_limbs_below_modulus(w + 6 * k)) return false;
    return true;
}
// r = the group order of G1 and G2: the scalar field's modulus (an instance value's raw limbs, in either encoding, must be below it)
__host__ __device__ inline bool fr_limbs_below_modulus(const uint64_t *c)
{
    constexpr uint64_t R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    for (int k = 3; k >= 0; k--) {
        if (c[k] < R[k]) return true;
        if (c[k] > R[k]) return false;
    }
    return false;
}
// ark-ff affine point (x | y, 6 x u64 each, x 2^384; all zero = the point at infinity) -> both forms used here
__host__ __device__ inline G1Affine29 g1_lazy_from_ark(const uint64_t *w)
{
    G1Affine29 p;
    uint64_t any = 0;
    for (int k = 0; k < 12; k++) any |= w[k];
    p.inf = any == 0;
    p.x = fq_canonical(fq_from_ark((const uint32_t *)w));
    p.y = fq_canonical(fq_from_ark((const uint32_t *)(w + 6)));
    return p;
}
__host__ __device__ inline pairing::G1 g1_strict(const G1Affine29 &p)
{
    pairing::G1 r;
    r.x.v = fq_canonical(p.x); r.y.v = fq_canonical(p.y); r.inf = p.inf;
    return r;
}
// r P = O?  A ladder over the 255 bits of r with the complete formulas of frw_fq29.h
template <class F> __host__ __device__ inline bool in_subgroup(const AffineT<F> &p)
{
    constexpr uint64_t R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    if (p.inf) return true;
    XyzzT<F> acc = pt_identity<F>();
#pragma nounroll
    for (int bit = 254; bit >= 0; bit--) {
        acc = pt_double(acc);
        if ((R[bit >> 6] >> (bit & 63)) & 1ull) acc = pt_add_affine(acc, p);
    }
    return acc.inf || F::is_zero(acc.zz);
}
// gamma_abc_g1[i] of a key (12 x u64): canonical limbs, on the curve, in the subgroup of order r
__host__ __device__ inline bool g1_point_valid(const uint64_t *w)
{
    if (!coordinates_canonical(w, 2)) return false;
    const G1Affine29 p = g1_lazy_from_ark(w);
    return pairing::g1_on_curve(g1_strict(p)) && in_subgroup(p);
}

// frw_groth16_vk_load_opts; check_gamma_abc = false leaves gamma_abc_g1's curve and subgroup checks to the caller (the device load
// has made them already; canonical limbs are still asked for here)
int vk_load(const uint64_t *vk, size_t num_instance, bool check_gamma_abc, frw_groth16_vk **out);

// the verification of one proof from its prepared inputs on: the proof points' checks, the pairing product.  prepared: the affine
// point gamma_abc_g1[0] + sum x_i gamma_abc_g1[i] in ark-ff's bytes (12 x u64, all zero = infinity).  1, 0 or -1 as frw_groth16_verify.
int verify_prepared(const frw_groth16_vk &vk, const uint64_t *prepared, const uint64_t *proof, int flags);

// fn(i) for every i < batch on up to 32 host threads (fewer if no more can be had); false if some fn threw
template <class Fn> bool for_each_proof(size_t batch, Fn fn)
{
    const size_t hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t threads = std::min<size_t>(std::min<size_t>(batch, hw), 32);
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    auto work = [&]() {
        try {
            for (size_t i; (i = next.fetch_add(1)) < batch;) fn(i);
        } catch (...) {
            failed = true;
        }
    };
    if (threads <= 1) work();
    else {
        std::vector<std::thread> pool;
        try {
            for (size_t t = 0; t < threads; t++) pool.emplace_back(work);
        } catch (...) {                                              // no more threads to be had: the ones there are finish the batch
            if (pool.empty()) work();
        }
        for (auto &t : pool) t.join();
    }
    return !failed;
}

}  // namespace verify
}  // namespace frw
