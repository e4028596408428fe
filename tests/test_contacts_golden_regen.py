"""CPU: tests/golden/contacts_*.npz are what tests/golden/make_contacts_golden.py makes of the unmodified reference (where
its library can be built), and they hold the situations they were made for."""
import importlib.util
import os

import numpy as np
import pytest

import contacts_util as cu

_spec = importlib.util.spec_from_file_location("make_contacts_golden", os.path.join(cu.HERE, "golden", "make_contacts_golden.py"))
mcg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mcg)


def test_the_cases_are_the_generators():
    assert tuple(mcg.cases()) == cu.CASES


@pytest.mark.parametrize("name", cu.CASES)
def test_golden_is_what_the_reference_gives(po, name):
    if not po.reference_available():
        pytest.skip("the reference is not present on this machine")
    res, g = mcg.generate(name), cu.load_case(name)
    assert sorted(res) == sorted(g)
    for k in res:
        assert np.array_equal(res[k], g[k]), (name, k)


@pytest.mark.parametrize("name", cu.CASES)
def test_golden_holds_its_situation(name):
    """the generator's own assertions on the committed file: the restatement's records of the pre-state add up to the
    reference's table bit for bit; all four walls, grains with 0, 1 and 3 contacts, the pair pulled apart until fn clamps to 0
    and the pair sheared into the Coulomb clamp in the two large cases; f2, ifm, zz left alone on the film step"""
    case, g = mcg.cases()[name], cu.load_case(name)
    counts = mcg.check_case(name, case, g)
    assert counts["touching_pairs"] > 0
    for k in ("r_mm", "x_mm", "y_mm"):
        assert np.array_equal(g[k], np.asarray(case[k], float)), (name, k)
    assert os.path.getsize(os.path.join(cu.HERE, "golden", name + ".npz")) < 64 * 1024
