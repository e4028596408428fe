"""CPU: the restatement of the Voronoi analysis (tests/voronoi_util.py) against what a radical tessellation is by other routes --
the areas fill the box, a complete cell does not depend on the cutoff, a point belongs to the grain of the smallest power, scipy's
Voronoi diagram, the symmetry of the Delaunay graph --, the prototype's figures the contract was written from, and
lbmdem_write_voronoi_files (include/lbmdem_hip.h), the host-only formatter, character for character. No device is touched."""
import math
import os
import subprocess

import numpy as np
import pytest

import voronoi_util as vu

SYMBOLS = ["lbmdem_voronoi_compute", "lbmdem_download_voronoi_grains", "lbmdem_voronoi_grains_device",
           "lbmdem_download_voronoi_faces", "lbmdem_write_voronoi", "lbmdem_set_voronoi_output", "lbmdem_write_voronoi_files"]
BOX = (0.0, 1.0, 0.0, 0.8)   # Mgx, Mdx, Mby, Mhy


@pytest.fixture(scope="module")
def scene():
    """1 025 random centres in a 1 x 0.8 box, equal and unequal discs, restated once per cutoff"""
    rng = np.random.default_rng(1)
    n = 1025
    x, y = rng.uniform(0.01, 0.99, n), rng.uniform(0.01, 0.79, n)
    mono = vu.Restatement(x, y, np.full(n, 0.005), BOX)
    poly = vu.Restatement(x, y, rng.uniform(0.003, 0.006, n), BOX)
    return dict(n=n, x=x, y=y, mono=mono, poly=poly)


def test_areas_fill_the_box_when_every_cell_is_complete(scene):
    for A, empty in ((scene["mono"], 0), (scene["poly"], 1)):   # (one small disc of the unequal ones has no cell: its power loses everywhere)
        R = A.at(0.15)
        g = R["grains"]
        assert R["counts"]["complete"] == R["counts"]["cells"] == scene["n"] - empty and g["nverts"].max() <= 12
        assert R["counts"]["empty"] == empty and R["counts"]["overflowed"] == R["counts"]["nonfinite_grains"] == 0
        total = 0.0
        for a in g["area"]:
            total += float(a)
        assert abs(total - 0.8) <= 2e-15 * 0.8
        has = g["area"] > 0
        assert (g["phi"][has] > 0).all() and np.allclose((g["phi"] * g["area"])[has], math.pi * A.r[has] ** 2, rtol=1e-15)
        # the faces' CSR: every face has a length, a grain face names another grain, the perimeter is the faces' sum
        assert R["foff"][-1] == len(R["fsrc"]) == R["counts"]["grain_faces"] + R["counts"]["wall_faces"]
        assert (R["flen"] > 0).all() and (R["fsrc"] >= -4).all() and (R["fsrc"] < scene["n"]).all()
        sums = np.array([R["flen"][a:b].sum() for a, b in zip(R["foff"][:-1], R["foff"][1:])])
        assert np.allclose(sums, g["perimeter"], rtol=1e-13, atol=0)


def test_complete_cells_do_not_depend_on_the_cutoff(scene):
    A = scene["poly"]
    big = A.at(0.15)["grains"]
    # (the prototype the contract was written from counted 38 and 666: it had no `nverts > 0` in the flag and so took the one
    # disc without a cell, R2 = 0, for complete)
    for rcut, complete in ((0.03, 37), (0.06, 665)):
        g = A.at(rcut)["grains"]
        done = (g["flags"] & vu.COMPLETE) > 0
        assert done.sum() == complete                     # the prototype's figures
        assert (np.abs(g["area"][done] - big["area"][done]) <= 1e-12 * big["area"][done]).all()
        assert np.array_equal(g["faces"][done], big["faces"][done])
        assert np.array_equal(g["walls"][done], big["walls"][done])


def inside(P, px, py, eps):
    """+1 inside the counter-clockwise polygon by more than eps, -1 outside by more than eps, 0 near an edge"""
    worst = math.inf
    m = len(P)
    for k in range(m):
        a, b = P[k], P[(k + 1) % m]
        ex, ey = b[0] - a[0], b[1] - a[1]
        length = math.hypot(ex, ey)
        if length == 0:
            continue
        worst = min(worst, (ex * (py - a[1]) - ey * (px - a[0])) / length)
    return 0 if abs(worst) <= eps else (1 if worst > 0 else -1)


def test_a_point_lies_in_the_cell_of_the_smallest_power(scene):
    A = scene["poly"]
    R = A.at(0.15)
    rng = np.random.default_rng(5)
    checked = 0
    for px, py in zip(rng.uniform(0, 1, 2000), rng.uniform(0, 0.8, 2000)):
        power = (A.x - px) ** 2 + (A.y - py) ** 2 - A.r ** 2
        order = np.argsort(power)
        side = inside(R["polys"][order[0]], px, py, 1e-9)
        if side == 0:
            continue
        assert side == 1, (px, py)
        assert inside(R["polys"][order[1]], px, py, 1e-9) <= 0
        checked += 1
    assert checked > 1900


def test_equal_discs_against_scipy(scene):
    spatial = pytest.importorskip("scipy.spatial")
    x, y, n = scene["x"], scene["y"], scene["n"]
    g = scene["mono"].at(0.15)["grains"]
    V = spatial.Voronoi(np.c_[x, y])
    checked = 0
    for i in range(n):
        reg = V.regions[V.point_region[i]]
        if -1 in reg or g["walls"][i] != 0:
            continue
        p = V.vertices[reg]
        if (p[:, 0] < 0).any() or (p[:, 0] > 1).any() or (p[:, 1] < 0).any() or (p[:, 1] > 0.8).any():
            continue
        a = 0.5 * abs(np.dot(p[:, 0], np.roll(p[:, 1], -1)) - np.dot(p[:, 1], np.roll(p[:, 0], -1)))
        assert abs(a - g["area"][i]) <= 1e-12 and len(reg) == g["faces"][i], i
        checked += 1
    assert checked == 931


def test_delaunay_graph_is_symmetric(scene):
    for A, rcut in ((scene["poly"], 0.15), (scene["poly"], 0.06), (scene["mono"], 0.15)):
        R = A.at(rcut)
        done = (R["grains"]["flags"] & vu.COMPLETE) > 0
        off, src = R["foff"], R["fsrc"]
        nb = [set(int(j) for j in src[off[i]:off[i + 1]] if j >= 0) for i in range(A.n)]
        for i in np.nonzero(done)[0]:
            for j in nb[i]:
                if done[j]:
                    assert int(i) in nb[j], (rcut, i, j)
        assert sum(len(s) for s in nb) == R["counts"]["grain_faces"]


def ring(m):
    th = 2 * np.pi * np.arange(m) / m
    return np.r_[0.5, 0.5 + 0.1 * np.cos(th)], np.r_[0.4, 0.4 + 0.1 * np.sin(th)], np.full(m + 1, 0.01)


def test_ring_of_neighbours_fills_and_overflows_the_polygon():
    g = vu.restate(*ring(28), BOX, 0.15)["grains"]
    assert g["nverts"][0] == 28 == g["faces"][0] and g["flags"][0] == vu.COMPLETE and g["walls"][0] == 0
    R = vu.restate(*ring(40), BOX, 0.15)
    g = R["grains"]
    assert g["flags"][0] == vu.OVERFLOW and R["counts"]["overflowed"] == 1 and R["foff"][1] == 0
    assert g["nverts"][0] == g["faces"][0] == g["walls"][0] == 0
    assert g["area"][0] == g["perimeter"][0] == g["phi"][0] == g["R2"][0] == 0.0


def nine(dd):
    a, c = 2.0 ** -9, 2.0 ** -6
    return (np.array([c, c + a, c - a, c, c, dd, c - a, c + a, c - a]), np.array([c, c, c, c + a, c - a, dd, c + a, c - a, c - a]),
            np.full(9, 2.0 ** -11))


def test_lattice_vertex_one_ulp_to_either_side():
    """a four-fold vertex: the diagonal neighbour's line passes through it, just inside it, or just outside"""
    a, c = 2.0 ** -9, 2.0 ** -6
    box = (0.0, 2.0 ** -5, 0.0, 2.0 ** -5)
    for dd, faces in zip((np.nextafter(c + a, -np.inf), c + a, np.nextafter(c + a, np.inf)), (5, 4, 4)):
        g = vu.restate(*nine(dd), box, 1.0)["grains"]
        assert g["faces"][0] == faces and g["area"][0] == a * a == 2.0 ** -18 and g["walls"][0] == 0, dd


def test_special_centres_in_the_restatement():
    x = np.array([0.2, 0.2, 0.6, np.nan, np.inf, 5.0, 0.5, 0.54, 0.58])
    y = np.array([0.3, 0.3, 0.3, 0.3, 0.3, -7.0, 0.6, 0.6, 0.6])
    r = np.array([0.01, 0.01, 0.01, 0.01, 0.01, 0.01, 0.05, 0.001, 0.05])
    R = vu.restate(x, y, r, BOX, 0.5)
    g = R["grains"]
    assert g["flags"][3] == g["flags"][4] == (vu.NONFINITE | vu.EMPTY) and R["counts"]["nonfinite_grains"] == 2
    assert g["area"][0] == g["area"][1] > 0                       # coincident centres do not cut each other
    assert g["flags"][7] == vu.EMPTY and g["nverts"][7] == 0      # a small disc between two large ones has no cell
    assert R["counts"]["empty"] == 3 and R["counts"]["cells"] == 6
    assert 7 not in R["fsrc"] and 8 in R["fsrc"][R["foff"][6]:R["foff"][7]]


def _results():
    rng = np.random.default_rng(9)
    x, y = rng.uniform(0.0, 1.0, 23), rng.uniform(0.0, 0.8, 23)
    x[5] = np.nan
    return vu.restate(x, y, rng.uniform(0.01, 0.03, 23), BOX, 0.5)


def test_files_are_exactly_the_expected_text(pkg, tmp_path):
    R = _results()
    rcut, t, W, H = 0.5, 0.125, 1.0, 0.8
    want = vu.files_text(R["grains"], rcut, R["counts"], t, W, H)
    for nfile in (7, 8):   # the second call appends its line to voronoi.data, without another header
        pkg.write_voronoi_files(str(tmp_path), nfile, R["grains"], rcut, R["counts"], t, W, H)
    assert (tmp_path / "voronoi000007.dat").read_text() == want[0]
    assert (tmp_path / "voronoi.data").read_text() == vu.DATA_HEADER + want[1] + want[1]
    assert sorted(os.listdir(tmp_path)) == ["voronoi.data", "voronoi000007.dat", "voronoi000008.dat"]
    lines = want[0].splitlines()
    assert lines[0] == "# rcut %e" % rcut and len(lines) == 2 + 23 and lines[2 + 5].split()[1:] == ["%e" % 0.0] * 3 + ["0", "0", "0", "10"]
    row = want[1].split()
    assert len(row) == 13 and int(row[1]) == 22 and float(row[9]) == pytest.approx(R["grains"]["area"].sum(), rel=1e-6)
    assert float(row[10]) == pytest.approx(0.8) and 0 < float(row[11]) < 1 and 3 <= float(row[12]) <= 8


def test_missing_directory_and_bad_cells_are_refused(pkg, tmp_path):
    R = _results()
    args = (0.5, R["counts"], 0.0, 1.0, 0.8)
    with pytest.raises(pkg.LbmDemError, match="cannot open"):
        pkg.write_voronoi_files(str(tmp_path / "not" / "there"), 0, R["grains"], *args)
    for field, i, v in (("nverts", 2, -1), ("nverts", 4, 33), ("faces", 1, -1), ("faces", 0, int(R["grains"]["nverts"][0]) + 1)):
        bad = R["grains"].copy()
        bad[field][i] = v
        with pytest.raises(pkg.LbmDemError, match=r"grain %d has -?\d+ faces on -?\d+ vertices, a cell has at most 32" % i) as e:
            pkg.write_voronoi_files(str(tmp_path), 0, bad, *args)
        assert e.value.code == -1
    for rcut in (0.0, float("nan"), float("inf")):
        with pytest.raises(pkg.LbmDemError, match="rcut must be finite and > 0"):
            pkg.write_voronoi_files(str(tmp_path), 0, R["grains"], rcut, *args[1:])
    assert os.listdir(tmp_path) == []      # refused before anything is written
    pkg.write_voronoi_files(str(tmp_path), 0, R["grains"], *args)
    assert len(os.listdir(tmp_path)) == 2


def test_host_driver_refuses_bad_voronoi_arguments(pkg):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "host", "lbmdem")
    run = lambda *a: subprocess.run([exe, "no_such_sample.data", *a], capture_output=True, text=True)
    out = run("--voronoi", "2e-3", "--gpus", "2")
    assert out.returncode != 0 and "--voronoi is a single-GPU mode" in out.stderr
    for bad in (("--voronoi",), ("--voronoi", "0"), ("--voronoi", "-1e-3"), ("--voronoi", "x")):
        out = run(*bad)
        assert out.returncode != 0 and "--voronoi RCUT" in out.stderr, bad


def test_both_libraries_export_the_symbols(pkg, tmp_path):
    assert pkg.VORONOI_DTYPE == vu.VORONOI_DTYPE and pkg.VORONOI_COUNTERS == vu.COUNTERS and len(vu.COUNTERS) == 8
    assert (pkg.VOR_COMPLETE, pkg.VOR_EMPTY, pkg.VOR_OVERFLOW, pkg.VOR_NONFINITE, pkg.VOR_MAXV) == (vu.COMPLETE, vu.EMPTY, vu.OVERFLOW,
                                                                                                     vu.NONFINITE, vu.MAXV)
    assert set(SYMBOLS) <= set(pkg.exported_symbols())
    assert os.path.exists(pkg.SP_LIB_PATH), "the single-precision library has not been built"
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    R = _results()      # the host-only call works in the float library too
    pkg.write_voronoi_files(str(tmp_path), 1, R["grains"], 0.5, R["counts"], 0.5, 1.0, 0.8, precision="f32")
    want = vu.files_text(R["grains"], 0.5, R["counts"], 0.5, 1.0, 0.8)
    assert (tmp_path / "voronoi000001.dat").read_text() == want[0]
    assert (tmp_path / "voronoi.data").read_text() == vu.DATA_HEADER + want[1]
