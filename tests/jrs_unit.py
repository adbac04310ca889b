"""TEST HARNESS — shared by the host and device tests of the JRS scalars and the interval operations
(tests/gpu_unit/jrs_test.hip): the two libraries' entries through ctypes, the fixture of exact values
(tests/golden/jrs_samples.npz, written by tests/golden/make_jrs_samples.py) and the checks
themselves, so that the CPU tests (host library, fesetround) and the GPU tests (device library, ocml
directed rounding) assert the same things."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = os.path.join(HERE, "gpu_unit")
FIXTURE = os.path.join(HERE, "golden", "jrs_samples.npz")
LD = np.longdouble
_vp = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(_vp)


class Lib:
    """libjrs_test.so (device=True) or libjrs_test_host.so"""

    def __init__(self, device):
        name = "libjrs_test.so" if device else "libjrs_test_host.so"
        if not os.path.exists(os.path.join(UNIT, name)):   # built by __graft_entry__.build(); cheap
            subprocess.run(["make", "-C", UNIT, name], check=True, capture_output=True)
        self.L = ctypes.CDLL(os.path.join(UNIT, name))

    def jrs(self, T, joint, q0, qd0, qdd0, s):
        q0, qd0, qdd0 = (np.ascontiguousarray(v, dtype=np.float64) for v in (q0, qd0, qdd0))
        n = len(q0)
        j = np.full(n, joint, dtype=np.int32)
        s = np.ascontiguousarray(s, dtype=np.int32)
        out = np.full((n, 13), np.nan)
        assert self.L.jrs_selftest(int(T), n, _p(q0), _p(qd0), _p(qdd0), _p(j), _p(s), _p(out)) == 0
        return out

    def ival(self, op, a, b):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        out = np.full(len(a), np.nan)
        assert self.L.ival_selftest(len(a), int(op), _p(a), _p(b), _p(out)) == 0
        return out

    def icos(self, lo, hi):
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        out = np.full((len(lo), 4), np.nan)
        assert self.L.icos_selftest(len(lo), _p(lo), _p(hi), _p(out)) == 0
        return out


_FX = None


def fixture():
    global _FX
    if _FX is None:
        _FX = dict(np.load(FIXTURE))
    return _FX


def _ld(pair):
    """(hi, lo) double pairs [..., 2] as long doubles"""
    return LD(pair[..., 0]) + LD(pair[..., 1])


# ---- JRS scalars ---------------------------------------------------------------------------------
# columns of the 13 doubles (reach.h JrsJoint)
COS, SIN, QD, QDA_E, QDD = 0, 3, 6, 9, 10


def jrs_outputs(lib):
    fx = fixture()
    c = fx["cases"]
    T, joint = int(fx["consts"][0]), int(fx["consts"][1])
    return lib.jrs(T, joint, c[:, 0], c[:, 1], c[:, 2], c[:, 3].astype(np.int32))


def slack_of(states):
    """16 * 2^-52 * max(1, |q0| + |qd0| + |qdd0|) per row of states [n, >= 3]: the round-to-nearest
    operations on the centres and the rounding of q0 + ... in the Bernstein differences"""
    return 16 * 2.0 ** -52 * np.maximum(1.0, np.abs(states[:, :3]).sum(axis=1))


def excess_of(out, kh, ex):
    """[n, p, 4] long double: |exact - (centre + slope * khat)| - |radius| for cos, sin, qd, qdd, of the
    13 doubles out [n, 13] at samples with khat kh [n, p] and exact values ex [n, p, 4] (long double)
    (<= slack: the scalars enclose the trajectory)"""
    kh = LD(kh)
    res = np.zeros(ex.shape, dtype=LD)
    for n, col in enumerate((COS, SIN, QD, QDD)):
        col_e = col + 2
        mid = LD(out[:, None, col]) + LD(out[:, None, col + 1]) * kh
        res[:, :, n] = np.abs(ex[:, :, n] - mid) - np.abs(LD(out[:, None, col_e]))
    return res


def check_enclosure(out, states, kh, ex, report):
    """the enclosure of any fixture's samples (states [n, >= 3] = q0, qd0, qdd0, ...; kh, ex as
    excess_of) and no NaN; report: a callable for the measured figures. Returns the worst excess
    [n, 4]"""
    assert np.all(np.isfinite(out)), ("non-finite JRS scalar", states[~np.isfinite(out).all(axis=1)][:5].tolist())
    slack = slack_of(states)
    worst = excess_of(out, kh, ex).max(axis=1).astype(np.float64)   # [n, 4]
    units = worst / slack[:, None]
    report(f"worst excess: cos {worst[:, 0].max():.3e} sin {worst[:, 1].max():.3e} qd {worst[:, 2].max():.3e} "
           f"qdd {worst[:, 3].max():.3e}; in units of the slack: {units.max(axis=0)}")
    bad = np.argwhere(worst > slack[:, None])
    assert bad.size == 0, (len(bad), [(states[i].tolist(), int(k), float(worst[i, k]), float(slack[i])) for i, k in bad[:5]])
    return worst


def jrs_slack():
    return slack_of(fixture()["cases"])


def jrs_excess(out):
    """excess_of on the samples of tests/golden/jrs_samples.npz"""
    fx = fixture()
    return excess_of(out, fx["points"][:, :, 1], _ld(fx["exact"]))


def check_jrs(out, report):
    """the enclosure and no NaN on tests/golden/jrs_samples.npz"""
    fx = fixture()
    check_enclosure(out, fx["cases"], fx["points"][:, :, 1], _ld(fx["exact"]), report)


# ---- directed operations -------------------------------------------------------------------------
OPS = ("add_dn", "add_up", "sub_dn", "sub_up", "mul_dn", "mul_up", "div_dn", "sqrt_dn", "sqrt_up")
DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny


def exact_value(op, a, b):
    """the exact result as a Fraction; for the roots the pair (radicand, None) handled by directed()"""
    a, b = Fraction(float(a)), Fraction(float(b))
    name = OPS[op]
    if name.startswith("add"):
        return a + b
    if name.startswith("sub"):
        return a - b
    if name.startswith("mul"):
        return a * b
    if name.startswith("div"):
        return a / b
    return a


def _round_fraction(x, up):
    """the largest double <= x (up False) or smallest double >= x of a Fraction in the normal range"""
    f = float(x)   # CPython rounds a Fraction to nearest correctly
    if Fraction(f) == x:
        return f
    if up:
        return f if Fraction(f) > x else math.nextafter(f, math.inf)
    return f if Fraction(f) < x else math.nextafter(f, -math.inf)


def _round_sqrt(a, up):
    """directed rounding of sqrt(a), a > 0 a double: integer square root of the radicand scaled by an
    even power of two so that the root carries more than 64 bits"""
    fr = Fraction(float(a))
    num, den = fr.numerator, fr.denominator
    # a = num / den, den a power of two; make den an even power
    e = den.bit_length() - 1
    if e % 2:
        num, e = num * 2, e + 1
    while num.bit_length() < 140:
        num, e = num * 4, e + 2
    r = math.isqrt(num)
    exact = r * r == num
    lo = Fraction(r, 2 ** (e // 2))
    if exact:
        return _round_fraction(lo, up), True
    # the root lies strictly between lo and lo + 2^-(e/2): both round the same way unless a double
    # sits between them, which 70 spare bits rule out
    hi = Fraction(r + 1, 2 ** (e // 2))
    d = _round_fraction(hi if up else lo, up)
    return d, False


def directed(op, a, b):
    """(expected double, exact Fraction or None, in_normal_range)"""
    up = OPS[op].endswith("up")
    if OPS[op].startswith("sqrt"):
        d, _ = _round_sqrt(a, up)
        return d, None, True
    x = exact_value(op, a, b)
    normal = x == 0 or (Fraction(DBL_MIN) <= abs(x) <= Fraction(DBL_MAX))
    if not normal:
        return None, x, False
    return _round_fraction(x, up), x, True


def operand_pairs(seed=11):
    """dict name -> (a, b) arrays: the operand families of the issue"""
    rng = np.random.default_rng(seed)
    n = 2000
    # 600 binades: exponents -300 .. 299, random signs and mantissas
    def rand(nn, emin=-300, emax=300):
        return (rng.choice([-1.0, 1.0], nn) * (1 + rng.random(nn)) * 2.0 ** rng.integers(emin, emax, nn))
    fam = {"random": (rand(n), rand(n))}
    # exactly representable results: small integers and dyadic fractions
    ia = rng.integers(-2 ** 20, 2 ** 20, 200).astype(np.float64)
    ib = rng.integers(1, 2 ** 20, 200).astype(np.float64) * rng.choice([-1.0, 1.0], 200)
    fam["exact"] = (np.concatenate([ia, ia * ib, ia * 0.125]), np.concatenate([ib, ib, np.full(200, 0.5)]))
    # results one ulp from a power of two
    p = 2.0 ** rng.integers(-40, 40, 100)
    below, above = np.nextafter(p, 0), np.nextafter(p, np.inf)
    fam["near_pow2"] = (np.concatenate([below, above, p, p * p, below * below, above * above]),
                        np.concatenate([np.full(100, 2.0 ** -80), -np.full(100, 2.0 ** -80), np.full(100, 2.0 ** -60),
                                        below, above, np.ones(100)]))
    fam["signed_zero"] = (np.array([0.0, -0.0, 0.0, -0.0, 1.5, -1.5, 0.0, -0.0]),
                          np.array([0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 3.0, -3.0]))
    # subnormal or overflowing quotients and products
    big, small = rand(100, 900, 1023), rand(100, -1022, -900)
    fam["range_edge"] = (np.concatenate([big, small, big, small, rand(50, -1022, -1000)]),
                         np.concatenate([big, small, small, big, rand(50, 40, 60)]))
    return fam


def check_directed(lib, report):
    """every directed operation on every family: tight in the normal range, enclosing outside it"""
    loose = 0
    bad = []   # collected, so that one run shows every operation that is off
    for name, (a, b) in operand_pairs().items():
        for op, opname in enumerate(OPS):
            if opname.startswith("sqrt"):
                aa = np.abs(a)
                aa = aa[(aa > 0) & np.isfinite(aa)]
                bb = np.zeros_like(aa)
            elif opname.startswith("div"):
                keep = b != 0
                aa, bb = a[keep], b[keep]
            else:
                aa, bb = a, b
            got = lib.ival(op, aa, bb)
            up = opname.endswith("up")
            for x, y, g in zip(aa, bb, got):
                want, exact, normal = directed(op, x, y)
                if normal:
                    if not g == want:
                        bad.append((name, opname, float(x).hex(), float(y).hex(), float(g).hex(), float(want).hex()))
                    continue
                # subnormal or beyond DBL_MAX: the enclosure only
                if math.isnan(g):
                    bad.append((name, opname, float(x).hex(), float(y).hex(), "nan", "enclosure"))
                    continue
                if up:
                    ok = g == math.inf or (math.isfinite(g) and Fraction(g) >= exact)
                else:
                    ok = g == -math.inf or (math.isfinite(g) and Fraction(g) <= exact)
                if not ok:
                    bad.append((name, opname, float(x).hex(), float(y).hex(), float(g).hex(), "enclosure"))
                    continue
                loose += 0 if _tight_outside(g, exact, up) else 1
    report(f"results outside the normal range that enclose without being tight: {loose}")
    assert not bad, (len(bad), sorted({(b[0], b[1]) for b in bad}), bad[:8])


def _tight_outside(g, exact, up):
    if math.isinf(g):
        return abs(exact) > Fraction(DBL_MAX) and (g > 0) == (exact > 0)
    n = math.nextafter(g, -math.inf if up else math.inf)
    if math.isinf(n):
        return True
    return (Fraction(n) < exact) if up else (Fraction(n) > exact)


# ---- icos / isin ---------------------------------------------------------------------------------
ULP1 = 2.0 ** -52


def icos_figures(lib):
    """(shortfall, extra width) [m, 2] (cos, sin) of the library's icos / isin on the fixture's
    intervals against the exact ranges: how far the result fails to enclose the exact range (0 when
    it encloses), and how much wider than the exact range it is"""
    fx = fixture()
    iv = fx["icos_intervals"]
    rng = _ld(fx["icos_range"])                   # [m, 4]: cos min, cos max, sin min, sin max
    out = lib.icos(iv[:, 0], iv[:, 1])
    assert np.all(np.isfinite(out))
    short = np.zeros((len(iv), 2))
    extra = np.zeros((len(iv), 2))
    for n in range(2):
        lo, hi = LD(out[:, 2 * n]), LD(out[:, 2 * n + 1])
        short[:, n] = np.maximum(0, np.maximum(lo - rng[:, 2 * n], rng[:, 2 * n + 1] - hi)).astype(np.float64)
        extra[:, n] = ((hi - lo) - (rng[:, 2 * n + 1] - rng[:, 2 * n])).astype(np.float64)
    return short, extra
