"""CPU: the restatement of the packing structure analysis (tests/structure_util.py) against what the definitions say directly,
the table of squared edges of lbmdem_structure_edges on the bits, and lbmdem_write_structure_files (include/lbmdem_hip.h), the
host-only formatter, character for character. No device is touched."""
import math
import os
import subprocess

import numpy as np
import pytest

import packing_util as pu
import structure_util as su

SYMBOLS = ["lbmdem_structure_edges", "lbmdem_structure_compute", "lbmdem_download_structure_grains",
           "lbmdem_structure_grains_device", "lbmdem_download_structure_hist", "lbmdem_download_structure_neighbours",
           "lbmdem_write_structure", "lbmdem_set_structure_output", "lbmdem_write_structure_files"]


def random_scene(rng, n):
    r = rng.uniform(0.3e-3, 0.9e-3, n)
    x, y = rng.uniform(0, 12e-3, n), rng.uniform(0, 9e-3, n)
    return x, y, r


def test_list_is_symmetric_and_ascending_and_the_histogram_holds_every_pair():
    rng = np.random.default_rng(4)
    for case in range(20):
        n = int(rng.integers(1, 90))
        x, y, r = random_scene(rng, n)
        rcut, nbins, shell = float(rng.choice([0.4e-3, 1.5e-3, 4e-3, 40e-3])), int(rng.choice([1, 7, 4096])), float(rng.choice([1.0, 1.2]))
        R = su.restate(x, y, r, rcut, nbins, shell)
        off, nbr = R["offsets"], R["nbr"]
        assert off[0] == 0 and off[-1] == len(nbr) == R["counts"]["entries"] == 2 * R["counts"]["pairs"]
        pairs = set()
        for i in range(n):
            seg = nbr[off[i]:off[i + 1]]
            assert (np.diff(seg) > 0).all() and i not in seg, case
            pairs.update((i, int(j)) for j in seg)
        assert all((j, i) in pairs for i, j in pairs), case
        assert R["hist"].sum() == R["counts"]["pairs"] and R["hist"].dtype == np.int64
        assert np.array_equal(R["grains"]["nb"], np.diff(off))
        assert (R["grains"]["bonds"] <= R["grains"]["nb"]).all()
        # every listed pair lies within rcut by another formula, and every pair that is clearly inside is listed
        d = np.hypot(x[None, :] - x[:, None], y[None, :] - y[:, None])
        assert all(d[i, j] <= rcut * (1 + 1e-12) for i, j in pairs)
        assert int(((d < rcut * (1 - 1e-12)) & ~np.eye(n, dtype=bool)).sum()) <= len(pairs)
        if rcut == 40e-3:
            assert R["counts"]["pairs"] == n * (n - 1) // 2 and R["counts"]["lone_grains"] == (1 if n == 1 else 0)


def test_special_centres_in_the_restatement():
    x = np.array([1e-3, 1e-3, 2e-3, np.nan, np.inf, 5.0])
    y = np.array([1e-3, 1e-3, 1e-3, 1e-3, 1e-3, -7.0])
    r = np.full(6, 0.5e-3)
    R = su.restate(x, y, r, 1.5e-3, 8, 1.2)
    c = R["counts"]
    assert c["coincident_pairs"] == 1 and c["nonfinite_grains"] == 2 and c["pairs"] == 3 and c["lone_grains"] == 3
    assert R["nbr"].tolist() == [1, 2, 0, 2, 0, 1] and R["offsets"].tolist() == [0, 2, 4, 6, 6, 6, 6]
    assert R["hist"][0] == 1 and R["hist"].sum() == 3
    g = R["grains"]
    assert g["bonds"].tolist() == [2, 2, 2, 0, 0, 0]              # a coincident partner is bonded and adds nothing to the sums
    assert (g["c6"][:2] == 1.0).all() and (g["s6"][:3] == 0.0).all() and g["c6"][2] == 2.0 and g["c2"][2] == 2.0


@pytest.mark.parametrize("rcut,nbins", [(2.0 ** -9, 4), (1.1e-3, 7), (3.3e-3, 4096), (0.7, 1), (1e-160, 4096), (3e150, 33)])
def test_edges_are_the_numpy_table_on_the_bits(pkg, rcut, nbins):
    e2 = pkg.structure_edges(rcut, nbins)
    want = su.edges(rcut, nbins)
    assert len(e2) == nbins + 1 and su.same_bits(e2, want)
    assert (np.diff(e2) >= 0).all() and e2[0] == 0.0 and e2[-1] == rcut * rcut
    spelled = [(float(k) * (rcut / nbins)) * (float(k) * (rcut / nbins)) for k in range(nbins)] + [rcut * rcut]
    assert su.same_bits(e2, np.array(spelled))


def test_edges_refuse_bad_parameters(pkg):
    for rcut, nbins in ((0.0, 4), (-1.0, 4), (float("nan"), 4), (float("inf"), 4), (1.0, 0), (1.0, 4097)):
        with pytest.raises(pkg.LbmDemError, match="rcut must be finite and > 0|nbins must lie in 1 .. 4096") as e:
            pkg.structure_edges(rcut, nbins)
        assert e.value.code == -1


def test_triangular_lattice_has_six_bonds_and_full_order():
    rmean = 0.35
    r, x, y = pu.tri_packing(127, 121, rmean, noise=0.0)
    n = len(r)
    assert n > 200
    R = su.restate(x, y, r, 1.1 * 2 * rmean, 7, 1.2)
    g = R["grains"]
    inside = (x > x.min() + 3 * rmean) & (x < x.max() - 3 * rmean) & (y > y.min() + 3 * rmean) & (y < y.max() - 3 * rmean)
    assert inside.sum() > 100
    assert (g["bonds"][inside] == 6).all() and (g["nb"][inside] == 6).all()
    psi = np.sqrt(g["c6"][inside] ** 2 + g["s6"][inside] ** 2) / 6.0
    assert np.abs(psi - 1.0).max() < 1e-12
    assert np.abs(np.hypot(g["c2"][inside], g["s2"][inside])).max() < 1e-12   # an isotropic shell has no fabric
    assert R["counts"]["six_bonds"] >= inside.sum()
    psi6, fabric = su.order_parameters(g)
    assert 0.5 < psi6 <= 1.0 + 1e-12 and fabric < 0.05


def _results():
    rng = np.random.default_rng(9)
    x, y, r = random_scene(rng, 23)
    x[4], y[4] = x[3], y[3]
    return su.restate(x, y, r, 2.2e-3, 7, 1.2)


def test_files_are_exactly_the_expected_text(pkg, tmp_path):
    R = _results()
    rcut, nbins, shell, t, W, H = 2.2e-3, 7, 1.2, 0.125, 25.6e-3, 20e-3
    want = su.files_text(R["grains"], rcut, nbins, shell, R["hist"], R["counts"], t, W, H)
    for nfile in (7, 8):   # the second call appends its line to structure.data, without another header
        pkg.write_structure_files(str(tmp_path), nfile, R["grains"], rcut, nbins, shell, R["hist"], R["counts"], t, W, H)
    assert (tmp_path / "structure000007.dat").read_text() == want[0]
    assert (tmp_path / "gr000007.dat").read_text() == want[1]
    assert (tmp_path / "structure.data").read_text() == su.DATA_HEADER + want[2] + want[2]
    assert sorted(os.listdir(tmp_path)) == sorted(["structure000007.dat", "gr000007.dat", "structure000008.dat", "gr000008.dat",
                                                   "structure.data"])
    lines = want[0].splitlines()
    assert lines[0] == "# rcut %e nbins %d shell %e" % (rcut, nbins, shell) and len(lines) == 2 + len(R["grains"])
    row = want[1].splitlines()[2 + 3].split()
    e2 = su.edges(rcut, nbins)
    n = len(R["grains"])
    assert row[:2] == ["3", "%e" % math.sqrt(e2[3])] and int(row[3]) == R["hist"][3]
    assert float(row[4]) == pytest.approx(R["hist"][3] / (n * (n - 1) / 2 * math.pi * (e2[4] - e2[3]) / (W * H)), rel=1e-6)
    # one grain: no pair, g is 0 and no NaN reaches the file
    one = np.zeros(1, su.STRUCTURE_DTYPE)
    counts = dict(zip(su.COUNTERS, (0, 0, 0, 0, 1, 0, 0, 0)))
    (tmp_path / "one").mkdir()
    pkg.write_structure_files(str(tmp_path / "one"), 0, one, rcut, 1, shell, [0], counts, 0.0, W, H)
    want1 = su.files_text(one, rcut, 1, shell, np.zeros(1, np.int64), counts, 0.0, W, H)
    assert (tmp_path / "one" / "gr000000.dat").read_text() == want1[1] and "nan" not in want1[1]
    assert (tmp_path / "one" / "structure.data").read_text() == su.DATA_HEADER + want1[2]


def test_missing_directory_and_bad_indices_are_refused(pkg, tmp_path):
    R = _results()
    args = (2.2e-3, 7, 1.2, R["hist"], R["counts"], 0.0, 25.6e-3, 20e-3)
    with pytest.raises(pkg.LbmDemError, match="cannot open"):
        pkg.write_structure_files(str(tmp_path / "not" / "there"), 0, R["grains"], *args)
    n = len(R["grains"])
    for field, i, v in (("nb", 2, -1), ("nb", 5, n), ("bonds", 1, -1), ("bonds", 0, int(R["grains"]["nb"][0]) + 1)):
        bad = R["grains"].copy()
        bad[field][i] = v
        with pytest.raises(pkg.LbmDemError, match=r"grain %d has -?\d+ neighbours and -?\d+ bonds among %d grains" % (i, n)) as e:
            pkg.write_structure_files(str(tmp_path), 0, bad, *args)
        assert e.value.code == -1
    hist = R["hist"].copy()
    hist[6] = -2
    with pytest.raises(pkg.LbmDemError, match="bin 6 holds -2 pairs"):
        pkg.write_structure_files(str(tmp_path), 0, R["grains"], 2.2e-3, 7, 1.2, hist, R["counts"], 0.0, 25.6e-3, 20e-3)
    with pytest.raises(pkg.LbmDemError, match="shell must be finite and >= 1"):
        pkg.write_structure_files(str(tmp_path), 0, R["grains"], 2.2e-3, 7, 0.5, R["hist"], R["counts"], 0.0, 25.6e-3, 20e-3)
    assert os.listdir(tmp_path) == []      # refused before anything is written
    pkg.write_structure_files(str(tmp_path), 0, R["grains"], *args)
    assert len(os.listdir(tmp_path)) == 3


def test_host_driver_refuses_bad_structure_arguments(pkg):
    """`lbmdem --structure RCUT` is refused with --gpus N, like --clusters, and for anything that is no cutoff; all of it before a
    file is read or a device looked for"""
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "host", "lbmdem")
    run = lambda *a: subprocess.run([exe, "no_such_sample.data", *a], capture_output=True, text=True)
    out = run("--structure", "2e-3", "--gpus", "2")
    assert out.returncode != 0 and "--structure is a single-GPU mode" in out.stderr
    for bad in (("--structure",), ("--structure", "0"), ("--structure", "-1e-3"), ("--structure", "x")):
        out = run(*bad)
        assert out.returncode != 0 and "--structure RCUT" in out.stderr, bad
    for bad in ("0", "4097", "x"):
        out = run("--structure", "2e-3", "--structure-bins", bad)
        assert out.returncode != 0 and "--structure-bins N" in out.stderr, bad
    out = run("--structure", "2e-3", "--structure-shell", "0.9")
    assert out.returncode != 0 and "--structure-shell S" in out.stderr


def test_both_libraries_export_the_symbols(pkg, tmp_path):
    assert pkg.STRUCTURE_DTYPE == su.STRUCTURE_DTYPE and pkg.STRUCTURE_COUNTERS == su.COUNTERS and len(su.COUNTERS) == 8
    assert set(SYMBOLS) <= set(pkg.exported_symbols())
    assert os.path.exists(pkg.SP_LIB_PATH), "the single-precision library has not been built"
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    # the two host-only calls work in the float library too
    assert su.same_bits(pkg.structure_edges(1.1e-3, 7, precision="f32"), su.edges(1.1e-3, 7))
    R = _results()
    pkg.write_structure_files(str(tmp_path), 1, R["grains"], 2.2e-3, 7, 1.2, R["hist"], R["counts"], 0.5, 25.6e-3, 20e-3,
                              precision="f32")
    want = su.files_text(R["grains"], 2.2e-3, 7, 1.2, R["hist"], R["counts"], 0.5, 25.6e-3, 20e-3)
    assert (tmp_path / "structure000001.dat").read_text() == want[0]
    assert (tmp_path / "structure.data").read_text() == su.DATA_HEADER + want[2]
