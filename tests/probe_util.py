"""Shared by the probe tests: the generator of tests/golden/probes_*.npz (its case list and its restatement of the
reference's diagnostic formulas) and the comparison of a recorded series with such a golden."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_probe_golden", os.path.join(HERE, "golden", "make_probe_golden.py"))
mpg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mpg)

CASES = mpg.cases()


def golden(name):
    return dict(np.load(os.path.join(HERE, "golden", name + ".npz")))


def same_series(got, want, row, rows=None, what=""):
    """every field of a probe_read() dict against the records `rows` (default: all) of a golden / a run_case() dict, bit
    for bit; `row` = the pressure row the handle recorded"""
    sel = slice(None) if rows is None else rows
    n = len(np.asarray(want["step"])[sel])
    assert len(got["step"]) == n, (what, len(got["step"]), n)
    for k in mpg.FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])[sel]
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.array_equal(a, b), (what, k, float(np.abs(a.astype(float) - b.astype(float)).max()))
    a, b = got["pressure_row"], want[f"pressure_row_{row}"][sel]
    assert np.array_equal(a, b), (what, "pressure_row", row, float(np.abs(a - b).max()))
