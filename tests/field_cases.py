"""The moduli the run-time-field tests share (tests/test_field_*.py, tests/test_gpu_field.py), and what Python says about them."""

BN254 = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001          # ninv32 = 0xefffffff: the -T[0] digit is wrong here
ED25519_L = (1 << 252) + 27742317777372353535851937790883648493                      # Curve25519's group order: general digit
PALLAS = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001         # 255 bits, limbs of all ones in `one`
BLS12_377 = 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001       # 253 bits, ninv32 = 0xffffffff
BLS12_381 = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001       # must reproduce FRW_ENC_MONTGOMERY
P25519 = (1 << 255) - 19                                                             # top of the range
LOW = (1 << 160) + 7                                                                 # bottom of the range; odd is all that is asked

MODULI = {"bn254": BN254, "ed25519_l": ED25519_L, "pallas": PALLAS, "bls12_377": BLS12_377, "bls12_381": BLS12_381,
          "2^255-19": P25519, "2^160+7": LOW}
REFUSED = {"zero": 0, "even": BN254 - 1, "2^160": 1 << 160, "2^255+1": (1 << 255) + 1}

# ark-bn254's published Montgomery one (FrParameters::R), = 2^256 mod p
BN254_ONE_LIMBS = (0xAC96341C4FFFFFFB, 0x36FC76959F60CD29, 0x666EA36F7879462E, 0x0E0A77C19A07DF2F)

Q = 12289
# the largest value the un-reduced NTT ladder can hold: sum_{k <= 10} 2^k q^(k+1) - 1 (falcon_ntt.rs:31-39), 160 bits
LADDER_MAX = sum((1 << k) * Q ** (k + 1) for k in range(11)) - 1


def consts(p):
    """what frw_field_info reports, from Python integers"""
    return {"one": (1 << 256) % p, "k1": (1 << 288) % p, "k5": (1 << 416) % p, "r2": (1 << 512) % p,
            "ninv32": (-pow(p, -1, 1 << 32)) % (1 << 32), "bits": p.bit_length()}


def mont(x, p):
    return x * (1 << 256) % p


def limbs4(x):
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
