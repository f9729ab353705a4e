"""Time the ways a Groth16 proving key of the Falcon NTT circuit comes into being, in one process (wall clock around each call; every call
synchronises the device itself):
  frw_groth16_setup                   the key made from toxic waste (until the wire format, the only way to get this key at all)
  frw_groth16_pk_to_wire_dev          the handle written out, compressed and uncompressed
  frw_groth16_pk_load                 from ark-ff limbs in host memory (the limbs are made here from the uncompressed bytes in Python
                                      integers; that conversion is not timed)
  frw_groth16_pk_load_wire_dev        compressed and uncompressed, each with every point's subgroup ladder (checked) and without (vouched)
One JSON object per line.  --trace-run: setup, one export and ONE checked compressed load only -- the run to put under
rocprofv3 --kernel-trace --stats for the per-kernel split.
usage: python tools/time_pk_wire.py [--logn 10] [--trace-run]"""
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
Q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
FQ_R = (1 << 384) % Q


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def limbs_of(run, coordinates):
    """uncompressed wire points (`coordinates` field elements of 48 bytes each, the flags in the last byte) -> ark-ff's Montgomery limbs"""
    out = bytearray()
    step = 48 * coordinates
    for off in range(0, len(run), step):
        pt = run[off:off + step]
        if pt[-1] & 0x40:
            out += bytes(step)
            continue
        for c in range(coordinates):
            out += (int.from_bytes(pt[48 * c:48 * c + 48], "little") * FQ_R % Q).to_bytes(48, "little")
    return np.frombuffer(bytes(out), dtype=np.uint64).reshape(-1, 6 * coordinates)


def main():
    logn = int(sys.argv[sys.argv.index("--logn") + 1]) if "--logn" in sys.argv else 10
    trace_run = "--trace-run" in sys.argv
    eng = frw.WitnessEngine(0)
    rng = random.Random(9)
    say = lambda **kw: print(json.dumps(kw), flush=True)
    (pk, vk), t = timed(lambda: eng.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5))))
    info = eng.groth16_pk_info(pk)
    ni = len(vk["gamma_abc_g1"])
    nv, n = int(info.z_hi) - 3, int(info.h_hi) + 1
    say(call="frw_groth16_setup", logn=logn, num_instance=ni, num_witness=nv - ni, domain_size=n, g1_points=ni + 2 + 2 * nv + n - 1 + nv - ni,
        g2_points=3 + nv, key_bytes=int(info.key_bytes), seconds=round(t, 4))
    wire = {}
    for compressed in ((True,) if trace_run else (True, False)):
        wire[compressed], t = timed(lambda: eng.groth16_pk_to_wire(pk, vk, compressed=compressed))
        say(call="frw_groth16_pk_to_wire_dev", compressed=compressed, bytes=len(wire[compressed]), seconds=round(t, 4))
    eng.groth16_pk_free(pk)
    if trace_run:
        (h, _), t = timed(lambda: eng.groth16_pk_load_wire(wire[True], compressed=True, checked=True, mode=frw.KEY_TABLES))
        say(call="frw_groth16_pk_load_wire_dev", compressed=True, checked=True, seconds=round(t, 4))
        eng.groth16_pk_free(h)
        eng.close()
        return
    # the same key as host limbs, for the loader the library had before
    raw = wire[False]
    o = frw.groth16_pk_wire_info(raw, compressed=False)
    fixed = 96 + 3 * 192 + 8 + ni * 96
    g1 = lambda off, count: limbs_of(raw[off:off + 96 * count], 2)
    g2 = lambda off, count: limbs_of(raw[off:off + 192 * count], 4)
    args = (ni, nv - ni, n, g1(0, 1), g1(fixed, 1), g1(fixed + 96, 1), g2(96, 1), g2(96 + 2 * 192, 1), g1(o["a_query_offset"], nv),
            g1(o["b_g1_query_offset"], nv), g2(o["b_g2_query_offset"], nv), g1(o["h_query_offset"], n - 1), g1(o["l_query_offset"], nv - ni))
    h, t = timed(lambda: eng.groth16_pk_load(*args, mode=frw.KEY_TABLES))
    say(call="frw_groth16_pk_load", source="host limbs", seconds=round(t, 4))
    eng.groth16_pk_free(h)
    for compressed in (True, False):
        for checked in (True, False):
            (h, _), t = timed(lambda: eng.groth16_pk_load_wire(wire[compressed], compressed=compressed, checked=checked, mode=frw.KEY_TABLES))
            say(call="frw_groth16_pk_load_wire_dev", compressed=compressed, checked=checked, seconds=round(t, 4))
            again, t = timed(lambda: eng.groth16_pk_to_wire(h, vk, compressed=compressed))
            say(call="frw_groth16_pk_to_wire_dev", of="the loaded key", compressed=compressed, equal_to_the_bytes_loaded=again == wire[compressed],
                seconds=round(t, 4))
            eng.groth16_pk_free(h)
    eng.close()


if __name__ == "__main__":
    main()
