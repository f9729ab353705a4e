"""The multi-scalar multiplication over a curve on a run-time Fq2 (frw_msmf2_*; falcon-r1cs_amd/csrc/frw_msm_field2.hip).  Every
comparison is exact, byte for byte.  Bases are Q_i = (s0 + i d) G (tests/curve2_reference.py), so the expected sum is ONE multiple of G;
tests/test_curve2_host.py holds that shortcut to direct double-and-add.  bn254_g2 is beta = -1; pallas_ext (beta = 5, group order
unknown: unreduced integer multiples) is the only cover of the general product.
  1. sizes over bn254_g2 and pallas_ext, 2^16 once       2. exceptional additions inside the kernels
  3. digit boundaries of plain integers, both window widths   4. chunking   5. graph replay
  6. the load-time check and the refusals   7. the example"""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import curve2_reference as R
import field_cases as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S0, D = 0x1234567, 0x89AB
SIZES = [1, 2, 3, 63, 64, 65, 1000]
G2, EXT = R.BN254_G2, R.PALLAS_EXT


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def bases(name, n):
    """the first n points of the curve's progression (the longest one made is shared: a prefix of a progression is a progression)"""
    longest = (1 << 16) if name == "bn254_g2" else 65
    if n < longest:
        return bases(name, longest)[:n]
    return tuple(R.progression(R.CURVES[name], n, S0, D))


@functools.lru_cache(maxsize=None)
def packed(name, n):
    longest = (1 << 16) if name == "bn254_g2" else 65
    if n < longest:
        return packed(name, longest)[:n]
    return R.pack(R.CURVES[name], bases(name, n))


def msm(engine, handle, c, ks, stride=None, montgomery=False, num_scalars=None, statements_of_workspace=None):
    """frw_msmf2_dev on a batch of scalar vectors (lists of integers, one per statement) -> the points, synchronised.  The stride's tail
    is filled with a value that would change the result if it were read; the workspace is exactly what the call is told."""
    import torch
    dev = torch.device("cuda:0")
    batch, n = len(ks), len(ks[0])
    stride = n if stride is None else stride
    num_scalars = n if num_scalars is None else num_scalars
    arr = np.full((batch, stride, 4), 0x0123456789ABCDEF, dtype=np.uint64)
    for s, row in enumerate(ks):
        if n:
            arr[s, :n] = R.scalars(row, c.r if montgomery else None)
    size = engine.msmf2_workspace_bytes(handle, batch if statements_of_workspace is None else statements_of_workspace)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    out = torch.full((batch, 16), -1, dtype=torch.int64, device=dev)
    engine.msmf2_dev(handle, batch, _dev(arr), stride, num_scalars, montgomery, out, ws, size, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return R.unpack(c, out.cpu().numpy().view(np.uint64)), out


def plain_sum(c, ks, pts):
    """sum k_i Q_i for arbitrary points, through Python's double-and-add (small cases only)"""
    acc = None
    for k, p in zip(ks, pts):
        acc = R.add(c, acc, R.mul(c, k % c.order if c.order else k, p))
    return acc


class Loaded:
    def __init__(self, engine, c, pts, flags=0):
        self.engine, self.c = engine, c
        arr = pts if isinstance(pts, np.ndarray) else R.pack(c, pts)
        self.handle = engine.msmf2_load(c.q, c.r, c.beta, c.b, arr, flags)

    def __enter__(self):
        return self.handle

    def __exit__(self, *exc):
        self.engine.msmf2_free(self.handle)


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------------------
def check_sizes(engine, c, n, cases):
    rng = random.Random(n)
    with Loaded(engine, c, packed(c.name, n)) as h:
        info = engine.msmf2_info(h)
        assert (int(info.num_points), int(info.bases_bytes)) == (n, 128 * n)
        assert (int(info.window_bits), int(info.num_windows)) == ((15, 18) if n >= 1 << 16 else (13, 20))
        assert int(info.workspace_bytes_per_statement) == engine.msmf2_workspace_bytes(h, 1) > 0
        for montgomery, num_scalars in cases:
            # (Montgomery form holds values below r; a plain scalar is any 256-bit integer where the sum needs no group order)
            top = c.r if montgomery or c.order else 1 << 256
            ks = [[rng.randrange(top) for _ in range(n)] for _ in range(3)]
            got, _ = msm(engine, h, c, ks, stride=n + 5, montgomery=montgomery, num_scalars=num_scalars)
            want = [R.progression_sum(c, row[:num_scalars], S0, D) for row in ks]
            assert got == want, (c.name, n, montgomery, num_scalars)
            if num_scalars == 0:
                assert got == [None] * 3


@pytest.mark.parametrize("n", SIZES)
def test_sizes_over_bn254_g2_against_python(engine, n):
    check_sizes(engine, G2, n, [(m, k) for m in (False, True) for k in sorted({0, 1, n - 1, n})])


@pytest.mark.parametrize("n", [1, 3, 65])
def test_sizes_over_an_extension_whose_nonresidue_is_not_minus_one(engine, n):
    check_sizes(engine, EXT, n, [(m, k) for m in (False, True) for k in sorted({0, 1, n - 1, n})])


def test_two_to_the_sixteen_points_take_the_wide_windows(engine):
    n = 1 << 16
    check_sizes(engine, G2, n, [(True, n), (False, n - 1)])


# ---- 2. exceptional additions inside the kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [G2, EXT], ids=lambda c: c.name)
def test_equal_bases_with_equal_scalars_add_a_point_to_itself(engine, c):
    p = bases(c.name, 8)[5]
    with Loaded(engine, c, [p] * 64) as h:
        for k in (1, 7, 0xDEADBEEFCAFE, c.r - 2):
            got, _ = msm(engine, h, c, [[k] * 64])
            assert got == [R.mul(c, 64 * k % c.order if c.order else 64 * k, p)], k


@pytest.mark.parametrize("c", [G2, EXT], ids=lambda c: c.name)
def test_a_bucket_passes_through_infinity_and_goes_on(engine, c):
    pts = bases(c.name, 40)
    p = pts[3]
    rng = random.Random(2)
    # Q, -Q, Q, -Q, ..., Q with one scalar: whatever order the sort leaves them in, the bucket meets its own negative (or itself)
    alternating = [p if i % 2 == 0 else R.neg(c, p) for i in range(65)]
    with Loaded(engine, c, alternating) as h:
        k = rng.randrange(c.r)
        got, _ = msm(engine, h, c, [[k] * 65, [k] * 64 + [0]])
        assert got == [R.mul(c, k, p), None]
    # pairs Q_i, -Q_i with a scalar per pair, then points that stand alone
    paired = [q for i in range(20) for q in (pts[i], R.neg(c, pts[i]))] + list(pts[20:40])
    with Loaded(engine, c, paired) as h:
        ks = [k for _ in range(20) for k in [rng.randrange(c.r)] * 2] + [rng.randrange(c.r) for _ in range(20)]
        got, _ = msm(engine, h, c, [ks], montgomery=True)
        assert got == [plain_sum(c, ks[40:], pts[20:40])]


def test_bases_that_are_infinity_and_scalars_that_are_zero(engine):
    c = G2
    pts = list(bases(c.name, 65))
    for i in (0, 7, 8, 64):
        pts[i] = None
    rng = random.Random(3)
    with Loaded(engine, c, pts) as h:
        ks = [rng.randrange(c.r) for _ in range(65)]
        live = [(k, p) for k, p in zip(ks, pts) if p is not None]
        got, _ = msm(engine, h, c, [ks, [0] * 65, [0] * 64 + [1]])
        assert got == [plain_sum(c, [k for k, _ in live], [p for _, p in live]), None, None]
    with Loaded(engine, c, [None] * 3) as h:
        assert msm(engine, h, c, [[5, 6, 7]])[0] == [None]


@pytest.mark.parametrize("n", [65, 1 << 16])
def test_one_populated_bucket_the_folds_running_sum_meets_itself(engine, n):
    c = G2
    with Loaded(engine, c, packed(c.name, n)) as h:
        info = engine.msmf2_info(h)
        cb, w = int(info.window_bits), int(info.num_windows)
        rows, want = [], []
        for j in (0, 1, w // 2, w - 2):
            for digit in (1, 2, 1 << (cb - 1)):                    # bucket 0, bucket 1, the largest bucket
                k = digit << (cb * j)
                assert k < 1 << 256
                rows.append([0, 0, k] + [0] * 62)
                want.append(R.mul(c, k % c.r, bases(c.name, n)[2]))
        got, _ = msm(engine, h, c, rows, num_scalars=65, stride=65)
        assert got == want


def test_one_heavy_bucket(engine):
    c = G2
    n = 1 << 12
    with Loaded(engine, c, packed(c.name, n)) as h:
        got, _ = msm(engine, h, c, [[5] * n])
        assert got == [R.progression_sum(c, [5] * n, S0, D)]


# ---- 3. digit boundaries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 1 << 16])
def test_digit_boundaries_of_plain_integers(engine, n):
    c = G2
    pts = bases(c.name, n)
    with Loaded(engine, c, packed(c.name, n)) as h:
        info = engine.msmf2_info(h)
        cb, w = int(info.window_bits), int(info.num_windows)
        assert cb * w >= 257 and (cb, w) == ((13, 20) if n == 3 else (15, 18))
        top = (1 << 256) - 1
        half = sum(1 << (cb - 1 + cb * j) for j in range(w)) & top                 # every digit 2^(C-1): stays, the largest bucket
        over = sum(((1 << (cb - 1)) + 1) << (cb * j) for j in range(w)) & top      # every digit 2^(C-1) + 1: a carry through all windows
        ks = [c.r - 1, c.r, c.r + 1, top, half, over, 0, 1]
        ks += [1 << (cb * j) for j in range(w)] + [(1 << (cb * j)) - 1 for j in range(w)]
        assert all(0 <= k <= top for k in ks)
        rng = random.Random(4)
        rows = [[k, rng.randrange(1 << 256), rng.randrange(1 << 256)] for k in ks]
        got, _ = msm(engine, h, c, rows, num_scalars=3, stride=4)
        assert got == [plain_sum(c, row, pts[:3]) for row in rows]
        alone, _ = msm(engine, h, c, [[k, 0, 0] for k in ks], num_scalars=3)
        assert alone == [R.mul(c, k % c.r, pts[0]) for k in ks]
        assert alone[1] is None and alone[0] == R.neg(c, pts[0]) and alone[3] == R.mul(c, top % c.r, pts[0])


def test_digit_boundaries_without_a_group_order(engine):
    c = EXT
    pts = bases(c.name, 3)
    with Loaded(engine, c, packed(c.name, 3)) as h:
        top = (1 << 256) - 1
        ks = [c.r - 1, c.r, top, 1 << 255, (1 << 13) - 1, 1 << 12, (1 << 12) + 1]
        got, _ = msm(engine, h, c, [[k, 1, 0] for k in ks], num_scalars=3)
        assert got == [R.add(c, R.mul(c, k, pts[0]), pts[1]) for k in ks]


# ---- 4. chunking, 5. graph ---------------------------------------------------------------------------------------------------------------
def test_a_workspace_of_one_statement_serves_a_batch_of_three(engine):
    import torch
    c = G2
    rng = random.Random(5)
    with Loaded(engine, c, packed(c.name, 1000)) as h:
        assert engine.msmf2_workspace_bytes(h, 1) < engine.msmf2_workspace_bytes(h, 2)
        ks = [[rng.randrange(c.r) for _ in range(1000)] for _ in range(3)]
        got_all, raw_all = msm(engine, h, c, ks, montgomery=True)
        got_one, raw_one = msm(engine, h, c, ks, montgomery=True, statements_of_workspace=1)
        assert torch.equal(raw_all, raw_one)
        assert got_one == [R.progression_sum(c, row, S0, D) for row in ks]


def test_the_call_is_captured_and_replays_on_changed_scalars(engine):
    import torch
    dev = torch.device("cuda:0")
    c = G2
    n = 1000
    rng = random.Random(6)
    with Loaded(engine, c, packed(c.name, n)) as h:
        size = engine.msmf2_workspace_bytes(h, 2)
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        scalars = torch.zeros((2, n, 4), dtype=torch.int64, device=dev)
        out = torch.zeros((2, 16), dtype=torch.int64, device=dev)
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            engine.msmf2_dev(h, 2, scalars, n, n, False, out, ws, size, side.cuda_stream)
        for _ in range(2):
            ks = [[rng.randrange(1 << 256) for _ in range(n)] for _ in range(2)]
            scalars.copy_(_dev(np.stack([R.scalars(row) for row in ks])))
            out.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            direct, raw = msm(engine, h, c, ks)
            assert torch.equal(out, raw)
            assert direct == [R.progression_sum(c, row, S0, D) for row in ks]


# ---- 6. the load-time check, the refusals -------------------------------------------------------------------------------------------------
def test_a_base_off_the_curve_refuses_the_load_and_is_named(engine):
    import falcon_r1cs_amd as frw
    c = G2
    n = 1000
    good = packed(c.name, n)
    for at in (0, n // 2, n - 1):
        bad = good.copy()
        bad[at, 12] ^= 1                                           # y.c1 with one bit flipped
        bad[n - 1, 0] ^= 2 if at != n - 1 else 0                   # a later bad base is not the one named
        with pytest.raises(frw.FrwError) as e:
            engine.msmf2_load(c.q, c.r, c.beta, c.b, bad)
        assert e.value.code == -1 and ("base %d " % at) in str(e.value), str(e.value)
        h = engine.msmf2_load(c.q, c.r, c.beta, c.b, bad, frw.MSMF_POINTS_ARE_CHECKED)
        assert int(engine.msmf2_info(h).num_points) == n
        engine.msmf2_free(h)
    big = good.copy()
    x = int.from_bytes(big[3, 4:8].tobytes(), "little") + c.q
    big[3, 4:8] = F.limbs4(x)                                      # x.c1: the same residue, not canonical
    with pytest.raises(frw.FrwError) as e:
        engine.msmf2_load(c.q, c.r, c.beta, c.b, big)
    assert "base 3 " in str(e.value)


def test_refusals(engine):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    lib = frw.load_library()
    c = EXT
    pts = bases(c.name, 8)
    for q, r, beta, b in ((c.q - 1, c.r, c.beta, c.b), (c.q, 1 << 160, c.beta, c.b), (c.q, c.r, 0, c.b), (c.q, c.r, c.q, c.b),
                          (c.q, c.r, c.beta, (0, 0)), (c.q, c.r, c.beta, (c.q, 1)), (c.q, c.r, c.beta, (1, c.q))):
        with pytest.raises(frw.FrwError) as e:
            engine.msmf2_load(q, r, beta, b, R.pack(c, pts))
        assert e.value.code == -1
    with pytest.raises(frw.FrwError):
        engine.msmf2_load(c.q, c.r, c.beta, c.b, np.zeros((0, 16), dtype=np.uint64))
    with pytest.raises(frw.FrwError) as e:
        engine.msmf2_load(c.q, c.r, c.beta, c.b, R.pack(c, pts), 2)
    assert "flags" in str(e.value)
    with Loaded(engine, c, pts) as h:
        per = engine.msmf2_workspace_bytes(h, 1)
        ws = torch.empty(per + 16, dtype=torch.uint8, device=dev)
        ks = _dev(R.scalars([1, 2, 3, 4, 5, 6, 7, 8]))
        out = torch.full((1, 16), 77, dtype=torch.int64, device=dev)
        P = lambda t: C.c_void_p(t.data_ptr())
        call = lambda hh, batch, s, stride, num, o, w, wb: lib.frw_msmf2_dev(hh, batch, s, stride, num, 0, o, w, wb, None)
        assert call(None, 1, P(ks), 8, 8, P(out), P(ws), per) == -1
        assert call(h, 1, None, 8, 8, P(out), P(ws), per) == -1
        assert call(h, 1, P(ks), 8, 8, None, P(ws), per) == -1
        assert call(h, 1, P(ks), 8, 8, P(out), None, per) == -1
        assert call(h, 1, P(ks), 8, 9, P(out), P(ws), per) == -1                               # more scalars than points
        assert call(h, 1, P(ks), 9, 9, P(out), P(ws), per) == -1
        assert call(h, 1, P(ks), 7, 8, P(out), P(ws), per) == -1                               # a stride below the scalars
        assert call(h, 1, P(ks), 8, 8, P(out), P(ws), per - 1) == -1                           # one byte short of a statement
        assert call(h, 1, P(ks), 8, 8, P(out), C.c_void_p(ws.data_ptr() + 8), per) == -1       # misaligned
        assert call(h, 0, None, 0, 0, None, None, 0) == 0                                      # batch = 0 touches nothing
        torch.cuda.synchronize()
        assert out.eq(77).all()
        assert call(h, 1, None, 0, 0, P(out), P(ws), per) == 0                                 # no scalars: infinity
        torch.cuda.synchronize()
        assert out.eq(0).all()
        assert call(h, 1, P(ks), 8, 8, P(out), P(ws), per) == 0
        torch.cuda.synchronize()
        assert R.unpack(c, out.cpu().numpy().view(np.uint64)) == [plain_sum(c, range(1, 9), pts)]
    engine.msmf2_free(None)


# ---- 7. the example ----------------------------------------------------------------------------------------------------------------------
def test_the_example_exits_zero():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "msm_bn254_g2.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert "== (sum z_i t_i) G" in res.stdout, res.stdout
