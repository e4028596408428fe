"""CPU: tests/golden/densities_*.npz are what tests/golden/make_densities_golden.py makes of the unmodified reference (where
its library can be built), and they hold the situations they were made for."""
import numpy as np
import pytest

import densities_util as du


@pytest.mark.parametrize("name", sorted(du.CASES))
def test_golden_is_what_the_reference_gives(po, name):
    if not po.reference_available():
        pytest.skip("the reference is not present on this machine")
    res, g = du.mdg.generate(name), dict(np.load(du.os.path.join(du.HERE, "golden", name + ".npz")))
    assert sorted(res) == sorted(g)
    for k in res:
        assert np.array_equal(res[k], g[k]), (name, k)


@pytest.mark.parametrize("name", sorted(du.CASES))
def test_golden_holds_its_situation(name):
    """the generator's own assertions on the committed file: grains on the map, moving fluid where the case has run, and a
    byte count for every file row of both sections that adds up to the file"""
    g, case = du.golden(name), du.CASES[name]
    du.mdg.check_case(name, case, g)
    head = len(du.mdg.header(case["lx"], case["ly"])) + len(du.mdg.VELOCITY_HEAD)
    assert int(g["row_bytes"].sum()) + head == int(g["vtk_bytes"])
    for s, key in enumerate(("p_row_%d", "v_row_%d")):
        for y in du.mdg.kept_rows(case["ly"]):
            assert len(g[key % y]) == int(g["row_bytes"][s, y]) and bytes(g[key % y]).count(b"\n") == case["lx"]
    assert int((g["hist_pressure"][:, 0] * g["hist_pressure"][:, 1]).sum()) == int(g["row_bytes"][0].sum())
    assert int((g["hist_velocity"][:, 0] * g["hist_velocity"][:, 1]).sum()) == int(g["row_bytes"][1].sum())
