"""The 224 polar BLER values the reference published (tests/golden/polar_bler_pins.json), re-run with
the batched simulation under the reference's stopping rule, one seeded device generator per pin.

The decoder is bit-exact with the reference's, so the only difference is the noise drawn; the bar is
the one tests/test_gpu_bler.py gives its bit-exact flooding decoder, two-sided:
|p - p_ref| <= 4 sqrt(q (1 - q) (1/n + 1/n_ref)) + 1/min(n, n_ref), q the pooled rate."""
import math

import pytest

from conftest import load_json

pytestmark = pytest.mark.gpu
PINS = load_json("polar_bler_pins.json")["pins"]


def test_pin_inventory():
    assert len(PINS) == 224
    assert {p["algo"] for p in PINS} == {"SC", "SC_optionB", "SCL", "SCL_optionB"}
    assert {p["L"] for p in PINS} == {1, 8, 16, 32} and len({tuple(p["testcase"]) for p in PINS}) == 15
    assert all(p["n_ref"] in (200, 400, 800, 2000) for p in PINS)


@pytest.mark.parametrize("i", range(len(PINS)),
                         ids=lambda i: "{}-L{}-K{}-N{}-{}dB".format(PINS[i]["algo"], PINS[i]["L"], PINS[i]["testcase"][0],
                                                                  PINS[i]["testcase"][1], PINS[i]["snr"]))
def test_pin(i):
    from python_5gtoolbox_amd import sim_polar
    pin = PINS[i]
    p, n = sim_polar.bler_point(pin["testcase"], pin["algo"], pin["L"], pin["snr"], seed=38212 + i)
    p_ref, n_ref = pin["bler"], pin["n_ref"]
    q = (p * n + p_ref * n_ref) / (n + n_ref)
    tol = 4 * math.sqrt(q * (1 - q) * (1 / n + 1 / n_ref)) + 1 / min(n, n_ref)
    print(f"pin {i}: {pin['algo']} L={pin['L']} {pin['testcase']} {pin['snr']} dB: {p:.5f} over {n} against "
          f"{p_ref:.5f} over {n_ref}, bar {tol:.5f}")
    assert abs(p - p_ref) <= tol
