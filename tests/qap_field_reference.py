"""Test helper: the R1CS -> QAP witness map over ANY prime field with a radix-2 domain, in Python integers -- oracle/qap.py with the
modulus p and the multiplicative generator g as arguments (ark-groth16 0.3.0 R1CStoQAP::witness_map over ark-poly 0.3.0's
Radix2EvaluationDomain, restated there).  Never imported by the product."""


def two_adicity(p):
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    return s, t


def two_adic_root(p, g):
    """(s, g^t) with p - 1 = 2^s t, t odd: ark-ff's TWO_ADICITY and TWO_ADIC_ROOT_OF_UNITY"""
    s, t = two_adicity(p)
    return s, pow(g, t, p)


class Domain:
    """Radix2EvaluationDomain::new(num_coeffs) over (p, g)"""

    def __init__(self, p, g, num_coeffs):
        size = 1
        while size < num_coeffs:
            size <<= 1
        self.p, self.g = p, g
        self.size = size
        self.log_size = size.bit_length() - 1
        s, root = two_adic_root(p, g)
        if self.log_size > s:
            raise ValueError("PolynomialDegreeTooLarge")
        for _ in range(self.log_size, s):                     # FftField::get_root_of_unity
            root = root * root % p
        self.group_gen = root
        self.group_gen_inv = pow(root, p - 2, p)
        self.size_inv = pow(size, p - 2, p)
        self.generator_inv = pow(g, p - 2, p)
        self.vanishing_inv = pow((pow(g, size, p) - 1) % p, p - 2, p)

    def _transform(self, vals, root):
        p, n = self.p, self.size
        a = list(vals) + [0] * (n - len(vals))
        L = self.log_size
        for i in range(n):                                    # bit reversal, then decimation in time
            j = int(format(i, "0%db" % L)[::-1], 2) if L else 0
            if i < j:
                a[i], a[j] = a[j], a[i]
        m = 2
        while m <= n:
            wm, half = pow(root, n // m, p), m // 2
            tw = [1] * half
            for k in range(1, half):
                tw[k] = tw[k - 1] * wm % p
            for k in range(0, n, m):
                for jj in range(half):
                    t = tw[jj] * a[k + jj + half] % p
                    u = a[k + jj]
                    a[k + jj] = (u + t) % p
                    a[k + jj + half] = (u - t) % p
            m <<= 1
        return a

    def fft(self, coeffs):
        return self._transform(coeffs, self.group_gen)

    def ifft(self, evals):
        return [v * self.size_inv % self.p for v in self._transform(evals, self.group_gen_inv)]

    def distribute_powers(self, coeffs, g):
        out, x = [], 1
        for c in coeffs:
            out.append(c * x % self.p)
            x = x * g % self.p
        return out

    def coset_fft(self, coeffs):
        return self.fft(self.distribute_powers(coeffs, self.g))

    def coset_ifft(self, evals):
        return self.distribute_powers(self.ifft(evals), self.generator_inv)


def witness_map(p, g, az, bz, cz, inputs):
    """h from A z, B z, C z (plain integers mod p) and the instance values `inputs` (the constant one first)"""
    nc, ni = len(az), len(inputs)
    d = Domain(p, g, nc + ni)
    pad = [0] * (d.size - nc)
    a = list(az) + pad
    a[nc:nc + ni] = [v % p for v in inputs]
    a = d.coset_fft(d.ifft(a))
    b = d.coset_fft(d.ifft(list(bz) + pad))
    c = d.coset_fft(d.ifft(list(cz) + pad))
    ab = [(x * y - z) * d.vanishing_inv % p for x, y, z in zip(a, b, c)]
    return d.coset_ifft(ab)


def lagrange_at(d, tau):
    """L_i(tau) for the domain's points w^i (tau outside the domain): (tau^n - 1) w^i / (n (tau - w^i)); and tau^n - 1"""
    p, n = d.p, d.size
    zt = (pow(tau, n, p) - 1) % p
    w, denom = 1, []
    for _ in range(n):
        denom.append((tau - w) % p)
        w = w * d.group_gen % p
    pref, acc = [], 1                                         # batch inversion
    for v in denom:
        pref.append(acc)
        acc = acc * v % p
    inv = pow(acc, p - 2, p)
    out = [0] * n
    for i in range(n - 1, -1, -1):
        out[i] = inv * pref[i] % p
        inv = inv * denom[i] % p
    w, scale = 1, zt * d.size_inv % p
    for i in range(n):
        out[i] = out[i] * w % p * scale % p
        w = w * d.group_gen % p
    return out, zt


def check_identity(p, g, az, bz, cz, inputs, h, tau):
    """A(tau) B(tau) - C(tau) == h(tau) (tau^n - 1), FFT-free; returns (lhs, rhs)"""
    nc, ni = len(az), len(inputs)
    d = Domain(p, g, nc + ni)
    assert len(h) == d.size
    lag, zt = lagrange_at(d, tau)
    a = list(az) + [v % p for v in inputs]
    at = sum(x * l for x, l in zip(a, lag)) % p
    bt = sum(x * l for x, l in zip(bz, lag)) % p
    ct = sum(x * l for x, l in zip(cz, lag)) % p
    ht = 0
    for c in reversed(h):
        ht = (ht * tau + c) % p
    return (at * bt - ct) % p, ht * zt % p
