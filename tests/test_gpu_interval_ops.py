"""The outward-rounded interval operations of armour-dev_amd/csrc/interval.h on the device
(__ocml_*_rtn/rtp_f64, and div_dn / sqrt_dn / sqrt_up from the round-to-nearest result and its fma
residual), through tests/gpu_unit/libjrs_test.so: the operands, exact references and bounds of
tests/test_interval_ops.py."""
import pytest

import jrs_unit as U
from test_interval_ops import check_icos

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    return U.Lib(device=True)


def test_device_directed_operations_are_tight(device):
    U.check_directed(device, print)


def test_device_icos_isin_enclose_the_exact_range(device):
    check_icos(device, print)
