"""CPU: the numpy restatement of the strain analysis (tests/strain_util.py) against what a deformation gradient and D2min must be,
before tests/test_gpu_strain.py holds the device to it on the bits, and lbmdem_write_strain_files (include/lbmdem_hip.h), the
host-only formatter, character for character. No device is touched.

The tolerances here are derived and apply to the restatement alone (the device is compared on bits). The scene is a 12 x 10 grid of
spacing 1 with a jitter of at most 1/4, cutoff 1.6: every grain has its axis neighbours (at most 1.5 away) and so a normal matrix Y
= sum d0 d0^T with both eigenvalues >= 1/2 (two neighbours at least 1/2 away along each axis) and <= 21 * 2.56 (at most 21
neighbours within 1.6): a condition number below 120. A fit F = X Y^-1 of an exactly affine field then carries a relative error of a
few hundred roundings of 2^-53 ~ 1e-16 each: below 1e-13, and 1e-9 is a bound with four decades to spare. A residual is then at most
1e-13 * rcut per neighbour, its square 1e-26 * rc2, and the sum over at most 21 neighbours below 1e-24 * rc2 -- 1e-20 * rc2 and
1e-18 * rc2 hold with room."""
import os
import subprocess

import numpy as np
import pytest

import strain_util as su

NX, NY, RCUT = 12, 10, 1.6
Q = 2.0 ** -12


@pytest.fixture(scope="module")
def mark():
    """the marked state: centres on multiples of 2^-12 (so that a translation by such a multiple is exact), angles, the list"""
    rng = np.random.default_rng(11)
    gx, gy = np.meshgrid(np.arange(1, NX + 1, dtype=float), np.arange(1, NY + 1, dtype=float))
    p = rng.permutation(gx.size)
    X0 = np.round((gx.ravel()[p] + rng.uniform(-0.25, 0.25, gx.size)) / Q) * Q
    Y0 = np.round((gy.ravel()[p] + rng.uniform(-0.25, 0.25, gx.size)) / Q) * Q
    T0 = rng.uniform(-3, 3, gx.size)
    off, nbr, rc2 = su.neighbour_list(X0, Y0, RCUT)
    deg = off[1:] - off[:-1]
    assert rc2 == RCUT * RCUT and deg.min() >= 2 and deg.max() <= 21
    return dict(X0=X0, Y0=Y0, T0=T0, off=off, nbr=nbr, rc2=rc2, n=len(X0), deg=deg)


def compute(M, x, y, th=None):
    return su.restate(M["X0"], M["Y0"], M["T0"], M["off"], M["nbr"], M["rc2"], x, y, M["T0"] if th is None else th)


def nbrs(M, i):
    return M["nbr"][M["off"][i]:M["off"][i + 1]]


def test_neighbour_list_is_symmetric_and_ascending(mark):
    M = mark
    pairs = set()
    for i in range(M["n"]):
        js = nbrs(M, i)
        assert (np.diff(js) > 0).all() and i not in js
        pairs |= {(i, int(j)) for j in js}
    assert all((j, i) in pairs for i, j in pairs) and len(pairs) == M["off"][-1]


def test_translation(mark):
    M = mark
    a, b = 3 * 2.0 ** -10, -5 * 2.0 ** -11
    R = compute(M, M["X0"] + a, M["Y0"] + b, M["T0"] + 0.25)
    g, c = R["grains"], R["counts"]
    assert (g["ux"] == a).all() and (g["uy"] == b).all()              # exact: every operand a multiple of 2^-12 below 2^4
    assert np.allclose(g["drot"], 0.25, rtol=0, atol=1e-15)
    assert (g["flags"] == 0).all() and c["fitted"] == M["n"] and c["lost"] == 0 and c["used"] == c["entries"] == M["off"][-1]
    for name, want in (("Fxx", 1.0), ("Fxy", 0.0), ("Fyx", 0.0), ("Fyy", 1.0)):
        assert np.abs(g[name] - want).max() < 1e-9, name
    assert g["d2min"].max() < 1e-20 * M["rc2"]
    assert np.array_equal(g["used"], M["deg"])


def test_affine_map(mark):
    M = mark
    A = np.array([[1.02, 0.03], [-0.01, 0.97]])
    x = A[0, 0] * M["X0"] + A[0, 1] * M["Y0"] + 0.125
    y = A[1, 0] * M["X0"] + A[1, 1] * M["Y0"] - 0.5
    g = compute(M, x, y)["grains"]
    assert (g["flags"] == 0).all()
    for name, want in (("Fxx", A[0, 0]), ("Fxy", A[0, 1]), ("Fyx", A[1, 0]), ("Fyy", A[1, 1])):
        assert np.abs(g[name] - want).max() < 1e-9, name
    assert (g["d2min"] / g["used"]).max() < 1e-18 * M["rc2"]
    D = su.derived(g)
    assert np.abs(D["exx"] - 0.02).max() < 1e-9 and np.abs(D["eyy"] + 0.03).max() < 1e-9
    assert np.abs(D["exy"] - 0.01).max() < 1e-9 and np.abs(D["omega"] + 0.02).max() < 1e-9
    assert np.abs(D["vol"] + 0.01).max() < 1e-9 and np.abs(D["dev"] - np.hypot(0.025, 0.01)).max() < 1e-9


def test_rigid_rotation(mark):
    M = mark
    phi = 0.1
    c, s = np.cos(phi), np.sin(phi)
    g = compute(M, c * M["X0"] - s * M["Y0"], s * M["X0"] + c * M["Y0"], M["T0"] + phi)["grains"]
    D = su.derived(g)
    assert np.abs(D["omega"] - s).max() < 1e-9 and np.abs(D["exy"]).max() < 1e-9
    assert np.abs(D["exx"] - (c - 1.0)).max() < 1e-9 and np.abs(D["eyy"] - (c - 1.0)).max() < 1e-9
    assert (g["d2min"] / g["used"]).max() < 1e-18 * M["rc2"]


def test_one_displaced_grain_in_an_affine_field(mark):
    """Grain p moves by delta on top of the affine map. Seen from p every neighbour is off by -delta, and the best F can only
    take out what is linear in d0: min over G of sum |delta + G d0_j|^2 = |delta|^2 (m - s^T Y^-1 s) with s = sum d0_j, m = used --
    positive by Cauchy-Schwarz unless the neighbours lie on a line that misses p. That number, from the marked geometry and the
    displacement alone, is what d2min[p] must be."""
    M = mark
    inner = np.nonzero((np.abs(M["X0"] - 6.5) < 1.5) & (np.abs(M["Y0"] - 5.5) < 1.5))[0]
    p = int(inner[0])
    radius = 0.4
    delta = np.array([0.5 * radius * np.cos(0.7), 0.5 * radius * np.sin(0.7)])
    A = np.array([[1.01, 0.02], [0.0, 0.99]])
    x = A[0, 0] * M["X0"] + A[0, 1] * M["Y0"]
    y = A[1, 0] * M["X0"] + A[1, 1] * M["Y0"]
    x[p] += delta[0]
    y[p] += delta[1]
    R = compute(M, x, y)
    g = R["grains"]
    js = nbrs(M, p)
    d0 = np.stack([M["X0"][js] - M["X0"][p], M["Y0"][js] - M["Y0"][p]], axis=1)
    s, Y = d0.sum(axis=0), d0.T @ d0
    want = float(delta @ delta) * (len(js) - float(s @ np.linalg.solve(Y, s)))
    assert want > 1e-3 * float(delta @ delta)                      # a positive bound, far above the 1e-18 * rc2 of the affine field
    assert g["d2min"][p] > 0.5 * want and g["d2min"][p] == pytest.approx(want, rel=1e-9)
    # a neighbour q of p sees one entry off by delta: |delta|^2 (1 - d^T Y_q^-1 d), d = X0_p - X0_q, the entry's leverage
    for q in js:
        dq = np.stack([M["X0"][nbrs(M, q)] - M["X0"][q], M["Y0"][nbrs(M, q)] - M["Y0"][q]], axis=1)
        d = np.array([M["X0"][p] - M["X0"][q], M["Y0"][p] - M["Y0"][q]])
        lev = float(d @ np.linalg.solve(dq.T @ dq, d))
        assert 0.0 < lev < 1.0 and g["d2min"][q] == pytest.approx(float(delta @ delta) * (1.0 - lev), rel=1e-9)
    group = np.r_[p, js]
    rest = np.setdiff1d(np.arange(M["n"]), group)
    assert g["d2min"][rest].max() < 1e-18 * M["rc2"] * 21
    assert R["counts"]["worst_grain"] == int(group[np.argmax(g["d2min"][group])])
    assert su.data_sums(g)[2] == g["d2min"][group].max()


def test_collinear_few_and_nonfinite():
    # three grains on a horizontal and three on a slanted line, two far from everything but each other, one alone
    X0 = np.array([1.0, 2.0, 3.0, 10.0, 10.5, 11.0, 20.0, 20.5, 30.0])
    Y0 = np.array([1.0, 1.0, 1.0, 10.0, 11.0, 12.0, 20.0, 20.0, 30.0])
    T0 = np.zeros(9)
    off, nbr, rc2 = su.neighbour_list(X0, Y0, 2.5)
    R = su.restate(X0, Y0, T0, off, nbr, rc2, X0 + 0.5, Y0 * 1.5, T0)
    g, c = R["grains"], R["counts"]
    assert (g["flags"][:6] == su.DEGENERATE).all() and (g["used"][:6] == 2).all()
    assert (g["flags"][6:8] == su.FEW).all() and (g["used"][6:8] == 1).all()
    assert g["flags"][8] == su.FEW and g["used"][8] == 0
    # (grains 3 and 5 are (1, 2) apart at the mark and (1, 3) afterwards: 10 > 2.5^2, lost at both ends)
    assert c == dict(fitted=0, few=3, degenerate=6, nonfinite_grains=0, entries=14, used=14, lost=2, worst_grain=-1)
    assert g["lost"].tolist() == [0, 0, 0, 1, 0, 1, 0, 0, 0]
    for name in ("Fxx", "Fxy", "Fyx", "Fyy", "d2min"):
        assert su.same_bits(g[name], np.zeros(9)), name
    assert (g["ux"] == 0.5).all() and su.same_bits(g["uy"], Y0 * 1.5 - Y0)
    assert su.data_sums(g)[1:] == (0.0, 0.0)


def test_nan_centre_is_flagged_and_skipped_by_its_neighbours(mark):
    M = mark
    x, y = M["X0"] + 0.0, M["Y0"] + 0.0
    bad = 17
    x[bad] = np.nan
    R = compute(M, x, y, M["T0"] + 1.0)
    g, c = R["grains"], R["counts"]
    assert g["flags"][bad] == su.NONFINITE and g["used"][bad] == 0 and g["lost"][bad] == 0
    for name in su.DOUBLES:
        assert su.same_bits(g[name][bad:bad + 1], [0.0]), name
    for j in nbrs(M, bad):
        assert g["used"][j] == M["deg"][j] - 1 and g["flags"][j] in (0, su.FEW, su.DEGENERATE)
    assert c["nonfinite_grains"] == 1 and c["entries"] == M["off"][-1] and c["used"] == c["entries"] - 2 * M["deg"][bad]
    # a mark with a NaN flags the grain as well; a neighbour's sums then carry the NaN and the fit is refused as degenerate
    X0 = M["X0"].copy()
    X0[bad] = np.nan
    g = su.restate(X0, M["Y0"], M["T0"], M["off"], M["nbr"], M["rc2"], M["X0"], M["Y0"], M["T0"])["grains"]
    assert g["flags"][bad] == su.NONFINITE and (g["flags"][nbrs(M, bad)] == su.DEGENERATE).all()
    assert (g["used"][nbrs(M, bad)] == M["deg"][nbrs(M, bad)]).all()


def test_a_grain_carried_away_is_lost_at_both_ends(mark):
    M = mark
    x, y = M["X0"] + 0.0, M["Y0"] + 0.0
    q = 40
    x[q] += 10 * RCUT
    g = compute(M, x, y)["grains"]
    far = np.hypot(x - x[q], y - y[q]) > RCUT
    assert far[nbrs(M, q)].all()
    assert g["lost"][q] == g["used"][q] == M["deg"][q]
    want = np.zeros(M["n"], int)
    want[nbrs(M, q)] = 1
    want[q] = M["deg"][q]
    assert np.array_equal(g["lost"], want)
    assert g["ux"][q] == x[q] - M["X0"][q] and g["d2min"][q] < 1e-20 * M["rc2"]      # its own neighbourhood moved rigidly


def test_worst_grain_takes_the_smaller_index_among_equals():
    # two mirror-image clusters far apart: the same d2min to the bit in both
    bx = np.array([0.0, 1.0, 0.0, -1.0, 0.0])
    by = np.array([0.0, 0.0, 1.0, 0.0, -1.0])
    X0, Y0 = np.r_[bx + 100.0, bx], np.r_[by, by]
    off, nbr, rc2 = su.neighbour_list(X0, Y0, 1.25)
    x, y = X0.copy(), Y0.copy()
    x[[1, 6]] += 0.25
    R = su.restate(X0, Y0, np.zeros(10), off, nbr, rc2, x, y, np.zeros(10))
    g = R["grains"]
    assert g["flags"][0] == g["flags"][5] == 0 and g["d2min"][0] == g["d2min"][5] > 0
    assert g["d2min"][0] == g["d2min"].max() and R["counts"]["worst_grain"] == 0


def test_files_are_exactly_the_expected_text(pkg, mark, tmp_path):
    M = mark
    rng = np.random.default_rng(5)
    x = 1.01 * M["X0"] + rng.normal(0, 0.02, M["n"])
    y = 0.98 * M["Y0"] + rng.normal(0, 0.02, M["n"])
    x[7] += 4.0
    y[30] = np.inf
    want_data = su.DATA_HEADER
    for nfile, (t, t_mark) in enumerate(((0.0, 0.0), (1.25e-3, 2.5e-4))):
        R = compute(M, x + 0.01 * nfile, y, M["T0"] + 0.3)
        assert R["counts"]["lost"] > 0 and R["counts"]["nonfinite_grains"] == 1 and R["counts"]["fitted"] > 100
        pkg.write_strain_files(str(tmp_path), nfile, R["grains"], M["rc2"], R["counts"], t, t_mark)
        a, b = su.files_text(R["grains"], M["rc2"], R["counts"], t, t_mark)
        want_data += b
        assert (tmp_path / ("strain%06d.dat" % nfile)).read_text() == a
        assert (tmp_path / "strain.data").read_text() == want_data
    msd, md2, big = su.data_sums(R["grains"])
    assert msd > 0 and md2 > 0 and big == R["grains"]["d2min"][R["counts"]["worst_grain"]] > 0


def test_missing_directory_and_bad_columns_are_refused(pkg, mark, tmp_path):
    M = mark
    R = compute(M, M["X0"] * 1.01, M["Y0"])
    args = (M["rc2"], R["counts"], 0.5, 0.25)
    with pytest.raises(pkg.LbmDemError, match="cannot open"):
        pkg.write_strain_files(str(tmp_path / "not" / "there"), 0, R["grains"], *args)
    for name, value, text in (("used", -1, r"grain 3 has lost \d+ of -1 neighbours used, of %d grains" % M["n"]),
                              ("used", M["n"], r"grain 3 has lost \d+ of %d neighbours used" % M["n"]),
                              ("lost", -1, r"grain 3 has lost -1 of \d+ neighbours used"),
                              ("lost", 22, r"grain 3 has lost 22 of \d+ neighbours used"),
                              ("flags", -1, r"grain 3 has flags -1, outside 0 \.\. 7"),
                              ("flags", 8, r"grain 3 has flags 8, outside 0 \.\. 7")):
        bad = R["grains"].copy()
        bad[name][3] = value
        with pytest.raises(pkg.LbmDemError, match=text):
            pkg.write_strain_files(str(tmp_path), 0, bad, *args)
        assert os.listdir(tmp_path) == []
    with pytest.raises(pkg.LbmDemError, match="counts must have eight values"):
        pkg.write_strain_files(str(tmp_path), 0, R["grains"], M["rc2"], [1, 2, 3], 0.5, 0.25)
    pkg.write_strain_files(str(tmp_path), 0, R["grains"], *args)
    assert sorted(os.listdir(tmp_path)) == ["strain.data", "strain000000.dat"]


def test_both_libraries_export_the_symbols(pkg, mark, tmp_path):
    names = ["lbmdem_strain_mark", "lbmdem_strain_clear", "lbmdem_strain_compute", "lbmdem_download_strain_grains",
             "lbmdem_strain_grains_device", "lbmdem_download_strain_reference", "lbmdem_write_strain", "lbmdem_set_strain_output",
             "lbmdem_write_strain_files"]
    assert set(names) <= set(pkg.exported_symbols())
    assert (pkg.STRAIN_NONFINITE, pkg.STRAIN_FEW, pkg.STRAIN_DEGENERATE) == (su.NONFINITE, su.FEW, su.DEGENERATE)
    assert pkg.STRAIN_DTYPE == su.STRAIN_DTYPE and pkg.STRAIN_COUNTERS == su.COUNTERS
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(names) <= exported, path
    # the float library's host-only formatter writes the same text
    M = mark
    R = compute(M, M["X0"] * 1.01, M["Y0"] + 0.125)
    pkg.write_strain_files(str(tmp_path), 1, R["grains"], M["rc2"], R["counts"], 0.5, 0.25, precision="f32")
    a, b = su.files_text(R["grains"], M["rc2"], R["counts"], 0.5, 0.25)
    assert (tmp_path / "strain000001.dat").read_text() == a and (tmp_path / "strain.data").read_text() == su.DATA_HEADER + b


def test_host_driver_refuses_bad_strain_arguments():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "2d-lbm-dem_amd", "host", "lbmdem")
    for args, text in ((["--strain"], "--strain RCUT"), (["--strain", "-1"], "--strain RCUT"), (["--strain", "x"], "--strain RCUT"),
                       (["--strain-incremental"], "--strain-incremental goes with --strain RCUT")):
        out = subprocess.run([exe, "nothing.data"] + args, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and text in out.stderr, (args, out.stderr[-300:])
