"""The outward-rounded interval operations of armour-dev_amd/csrc/interval.h, host side (fesetround; the
side the emulation runs), through tests/gpu_unit/libjrs_test_host.so.

Directed operations against exact arithmetic (fractions.Fraction; math.isqrt on scaled integers for
the roots): a _dn result must be the largest double <= the exact value, an _up result the smallest
double >= it, on 2000 random pairs over 600 binades, pairs with exactly representable results, results
one ulp from a power of two, signed zeros, and products / quotients that are subnormal or overflow
(there: the enclosure only, and the count of results that are not tight is reported).

icos / isin against the exact range of cos / sin over intervals of width 1e-3 .. 0.2 and +-1e-15
around every start angle of tests/test_jrs_enclosure.py (tests/golden/jrs_samples.npz, mpmath):
  * the result encloses the exact range up to E_HOST + 2 ulp(1): the end values come from the maths
    library's round-to-nearest cos, not from a directed one, so an end can fall short by its error;
  * the result is at most 1e-12 wider than the exact range.
"""
import pytest

import jrs_unit as U

# worst shortfall of the host build's icos / isin on these intervals, measured 2026-10-20 (ROCm clang,
# glibc libm, x86-64): 4.35e-17 (cos 4.30e-17, sin 4.34e-17), less than half an ulp of 1. Widest extra
# width: cos 1.7e-13, sin 4.4e-13 (both at q0 = -999.9, from the directed products of the reduction).
E_HOST = 4.35e-17
MAX_EXTRA = 1e-12


@pytest.fixture(scope="module")
def host():
    return U.Lib(device=False)


def test_host_directed_operations_are_tight(host):
    U.check_directed(host, print)


def check_icos(lib, report):
    short, extra = U.icos_figures(lib)
    report(f"icos / isin worst shortfall {short.max(axis=0)}, widest extra width {extra.max(axis=0)}")
    assert short.max() <= E_HOST + 2 * U.ULP1, short.max()
    assert extra.max() <= MAX_EXTRA, extra.max()
    return short.max()


def test_host_icos_isin_enclose_the_exact_range(host):
    worst = check_icos(host, print)
    assert worst <= E_HOST, f"E_HOST is out of date: the host build's worst shortfall is {worst:.3e}"
