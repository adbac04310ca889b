"""The reduce-scatter sum (wave.h scatter_sum) against the butterfly (wave_sum) in numpy, lane by lane:
the scatter computes each node of the butterfly's tree once, as own + partner where the butterfly has
own + partner on one lane and partner + own on the other, so every total has the butterfly's bits.
Data of mixed signs and magnitudes 1e-30 .. 1e30 is sensitive to the association: summing the levels
in the reverse order changes most totals, so equality here is not an accident of tame data."""
import numpy as np
import pytest

import reduce_model as M

WIDTHS = (1, 2, 7, 17, 19, 37, 55, 58, 62, 64)
DRAWS = 200


def draw(rng, N, draws=DRAWS):
    """[draws, 64 lanes, N]"""
    shape = (draws, M.LANES, N)
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-30, 30, shape)


@pytest.mark.parametrize("N", WIDTHS)
def test_scatter_has_the_butterflys_bits(N):
    v = draw(np.random.default_rng(N), N)
    ref = M.butterfly(np.swapaxes(v, -1, -2))[..., 0]   # [draws, N]
    assert np.array_equal(M.bits(M.scatter_totals(v)), M.bits(ref))
    # every lane that ends with an index holds that index's total, not only the storing lane
    r, P = M.scatter_sum(v)
    idx = np.array([M.scatter_index(P, l) for l in range(M.LANES)])
    ok = idx < N
    assert np.array_equal(M.bits(r[:, ok]), M.bits(ref[:, idx[ok]]))


@pytest.mark.parametrize("N", (19, 37, 55))
def test_scatter_with_dead_slots(N):
    """the call sites' max / min slots are not live in the scatter: the live totals keep their bits"""
    live = {19: [k >= 2 for k in range(19)], 37: [k != 36 for k in range(37)],
            55: [not (7 <= k <= 9 or k == 54) for k in range(55)]}[N]
    v = draw(np.random.default_rng(100 + N), N, 20)
    ref = M.butterfly(np.swapaxes(v, -1, -2))[..., 0]
    got = M.scatter_totals(v, live)
    assert np.array_equal(M.bits(got[:, live]), M.bits(ref[:, live]))


def test_index_map():
    for N in WIDTHS:
        P = M.scatter_width(N)
        assert P >= N and (P & (P - 1)) == 0 and (P == 1 or P // 2 < N)
        idx = [M.scatter_index(P, l) for l in range(P)]
        assert sorted(idx) == list(range(P))  # lanes 0 .. P-1 hold each index once
        k = P.bit_length() - 1
        assert idx == [int(format(l, f"0{k}b")[::-1], 2) if k else 0 for l in range(P)]  # the k-bit reversal
        # the higher lanes repeat the map of their low bits
        assert all(M.scatter_index(P, l) == idx[l & (P - 1)] for l in range(M.LANES))
    assert [M.scatter_index(64, l) for l in (1, 2, 32, 33, 63)] == [32, 16, 1, 33, 63]


def test_the_data_is_sensitive_to_the_association():
    rng = np.random.default_rng(5)
    v = draw(rng, 1)[..., 0]
    fwd = M.butterfly(v)[:, 0]
    rev = M.butterfly(v, levels=M.LEVELS[::-1])[:, 0]
    differ = np.mean(M.bits(fwd) != M.bits(rev))
    assert differ > 0.25, differ
