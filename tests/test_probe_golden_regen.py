"""CPU: tests/golden/probes_*.npz are what tests/golden/make_probe_golden.py makes of the unmodified reference (where its
library can be built), and the same formulas over the in-repo oracle give the same records -- so the GPU tests may check
against either."""
import numpy as np
import pytest

import probe_util as pu


@pytest.mark.parametrize("name", sorted(pu.CASES))
def test_golden_is_what_the_reference_gives(po, name):
    if not po.reference_available():
        pytest.skip("the reference is not present on this machine")
    res, g = pu.mpg.generate(name), pu.golden(name)
    assert sorted(res) == sorted(g)
    for k in res:
        assert np.array_equal(res[k], g[k]), (name, k)


@pytest.mark.parametrize("name", sorted(pu.CASES))
def test_oracle_gives_the_golden(po, name):
    case, g = pu.CASES[name], pu.golden(name)
    r, x1, x2 = pu.mpg.grains_m(case)
    res = pu.mpg.run_case(po.Oracle(case["lx"], case["ly"], r, x1, x2), case)
    assert sorted(res) == sorted(g)
    for k in res:
        assert np.array_equal(res[k], g[k]), (name, k)


@pytest.mark.parametrize("name", sorted(pu.CASES))
def test_golden_hits_every_branch(name):
    """the velocity profile crosses grains (the g[obst].v2 / c branch), a recorded pressure row crosses grains (the 0.0
    branch) and fluid (the other one), in the golden itself"""
    case, g = pu.CASES[name], pu.golden(name)
    assert len(g["step"]) == case["fluid_steps"] and np.all(np.diff(g["step"]) > 0)
    assert np.all(g["velocity_on_grain"] > 0) and np.all(g["velocity_on_grain"] < case["lx"])
    crossing = case["pressure_rows"][1]
    assert np.all(g[f"pressure_solid_{crossing}"] > 0)
    assert np.all((g[f"pressure_row_{crossing}"] != 0.0).sum(axis=1) > 0)
    assert np.any(g["point_pressure"] == 0.0) and np.any(g["point_pressure"] != 0.0)
    assert np.any(g["velocity_row"] != 0.0)
