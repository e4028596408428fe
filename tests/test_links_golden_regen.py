"""CPU: tests/golden/links_*.npz are what tests/golden/make_links_golden.py makes of the unmodified reference (where its
library can be built), and they hold the situations they were made for."""
import numpy as np
import pytest

import links_util as lu


@pytest.mark.parametrize("name", sorted(lu.CASES))
def test_golden_is_what_the_reference_gives(po, name):
    if not po.reference_available():
        pytest.skip("the reference is not present on this machine")
    res, g = lu.mlg.generate(name), dict(np.load(lu.os.path.join(lu.HERE, "golden", name + ".npz")))
    assert sorted(res) == sorted(g)
    for k in res:
        assert np.array_equal(res[k], g[k]), (name, k)


@pytest.mark.parametrize("name", sorted(lu.CASES))
def test_golden_holds_its_situation(name):
    """the generator's own assertions (stale entries: none in the clean cases, some in the overlap case; clipped discs,
    the one-node gap, the three-disc act case) on the committed file"""
    g = dict(np.load(lu.os.path.join(lu.HERE, "golden", name + ".npz")))
    stale = lu.mlg.check_case(name, lu.CASES[name], g)
    assert (stale == 0) == lu.CASES[name]["clean"]
    for k in ("r_mm", "x_mm", "y_mm"):
        assert np.array_equal(g[k], np.asarray(lu.CASES[name][k], float)), (name, k)
