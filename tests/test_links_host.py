"""CPU: the host side of the boundary-link export (include/lbmdem_hip.h: lbmdem_geometry_stats, lbmdem_download_act,
lbmdem_download_links, lbmdem_download_geometry_obst, lbmdem_write_obst, lbmdem_write_obst_files) -- the symbols, the one
formatter against the reference's three format strings, the link definition proven on the oracle before any GPU run, and the
error paths that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import links_util as lu

SYMBOLS = ("lbmdem_geometry_stats", "lbmdem_download_act", "lbmdem_download_links", "lbmdem_download_geometry_obst",
           "lbmdem_write_obst", "lbmdem_write_obst_files")


def test_symbols_in_header_and_library(pkg):
    declared = pkg.exported_symbols()
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
    assert "struct lbmdem_link { int x, y, q, grain; double delta; }" in open(pkg.HEADER_PATH).read()
    assert pkg.LINK_DTYPE.itemsize == 24 and pkg.LINK_DTYPE == lu.mlg.LINK_DTYPE


@pytest.mark.parametrize("name", sorted(lu.CASES))
def test_formatter_writes_the_references_text(pkg, tmp_path, name):
    g = lu.golden(name)
    pkg.write_obst_files(str(tmp_path), g["obst"], g["act"], g["links"])
    got = lu.read_files(tmp_path)
    eff = g["links"]
    assert got[0] == lu.map_text(g["obst"])
    assert got[1] == lu.map_text(g["act"])
    assert got[2] == lu.links_text(eff["x"], eff["y"], np.abs(eff["q"]), eff["delta"])
    if lu.CASES[name]["clean"]:   # the reference's own file: every non-zero delta entry, character for character
        assert got[2] == lu.links_text(g["delta_x"], g["delta_y"], g["delta_q"], g["delta_v"])
        assert got[2].count("\n") == len(g["delta_v"])
    else:
        assert got[2].count("\n") < len(g["delta_v"])


def test_formatter_skips_a_zero_delta(pkg, tmp_path):
    links = np.zeros(3, pkg.LINK_DTYPE)
    links["x"], links["y"], links["q"], links["delta"] = (3, 4, 5), (1, 1, 2), (2, -6, 8), (0.25, 0.0, 1.0)
    m = np.zeros((7, 5), np.int32)
    pkg.write_obst_files(str(tmp_path), m - 1, m, links)
    assert lu.read_files(tmp_path)[2] == "3  1  2  0.250000\n5  2  8  1.000000\n"


@pytest.mark.parametrize("name", sorted(lu.CASES))
def test_oracle_gives_the_golden(po, name):
    case, g = lu.CASES[name], lu.golden(name)
    r, x1, x2 = lu.mlg.grains_m(case)
    ora = po.Oracle(case["lx"], case["ly"], r, x1, x2)
    lu.mlg.drive(ora, case)
    assert np.array_equal(ora.get_obst(), g["obst"])
    assert np.array_equal(ora.get_act(), g["act"])
    lu.same_links(lu.mlg.effective_links(ora.get_obst(), ora.get_act(), ora.get_delta(), len(r)), g["links"], name)
    assert np.array_equal(ora.get_grains(), g["grains"])


def test_census_of_the_goldens():
    """the six counters are consistent: every slot of an active node is a link or a reset, every link near, far or neither"""
    for name in lu.CASES:
        c = lu.golden(name)["census"]
        assert c[0] >= c[1] > 0 and c[2] + c[5] == 8 * c[1] and c[3] + c[4] <= c[2] and c[3] > 0 and c[4] > 0, (name, c)


def test_error_paths_without_a_device(pkg, tmp_path):
    lib = pkg.load_library()
    g = lu.golden("links_La_37x50")
    links = np.ascontiguousarray(g["links"])
    obst, act = np.ascontiguousarray(g["obst"]), np.ascontiguousarray(g["act"])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    d = os.fsencode(str(tmp_path))
    assert lib.lbmdem_write_obst_files(d, 37, 50, None, vp(act), vp(links), len(links)) == -1
    assert lib.lbmdem_write_obst_files(d, 37, 50, vp(obst), None, vp(links), len(links)) == -1
    assert lib.lbmdem_write_obst_files(d, 37, 50, vp(obst), vp(act), None, len(links)) == -1
    assert lib.lbmdem_write_obst_files(d, 37, 50, vp(obst), vp(act), None, 0) == 0      # (no links: no list needed)
    missing = os.fsencode(str(tmp_path / "no" / "such" / "directory"))
    assert lib.lbmdem_write_obst_files(missing, 37, 50, vp(obst), vp(act), vp(links), len(links)) == -1
    assert b"cannot open" in lib.lbmdem_last_error()
    with pytest.raises(pkg.LbmDemError):
        pkg.write_obst_files(str(tmp_path), g["obst"], g["act"][:-1], g["links"])
    n = C.c_long(0)
    for rc in (lib.lbmdem_geometry_stats(None, vp(np.zeros(6, np.int64))), lib.lbmdem_download_act(None, vp(act)),
               lib.lbmdem_download_links(None, None, 0, C.byref(n)), lib.lbmdem_download_geometry_obst(None, vp(obst)),
               lib.lbmdem_write_obst(None, d)):
        assert rc == -1
