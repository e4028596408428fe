"""CPU: the specification of the time-averaged flow statistics -- the numpy restatement of tests/mean_util.py -- pinned to what can
be derived, and the host-only half of the feature: lbmdem_write_mean_files against bytes assembled here, the refusals that need no
device, the symbols of both libraries, the host driver's option. No device is touched.

What can be derived. A chain S = (((+0.0 + v) + v) + ...) of n equal addends:
  n = 1, 2   exact: v, 2v.
  n = 4      exact for EVERY double v (no overflow): fl(3v) differs from 3v by at most a quarter of ulp(4v) -- 3v needs one or two
             bits more than v, and in either case what is dropped is at most ulp(v) -- so fl(fl(3v) + v) = 4v.
  n = 8, ... not exact in general (fl(5v), fl(7v) may each be off by half an ulp(8v)); exact when v has so few significant bits
             that every partial sum is representable. The cases below with n >= 8 use such values (multiples of 2^-12 below 8).
Where S = n v exactly, S / n = v exactly (the quotient is representable), so mux == v; and with Sxx = n fl(v v) exactly,
rxx = fl(v v) - fl(mux mux) = +0.0."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mean_util as mu

SYMBOLS = ("lbmdem_mean_begin", "lbmdem_mean_sample", "lbmdem_mean_reset", "lbmdem_mean_end", "lbmdem_mean_stats",
           "lbmdem_mean_download", "lbmdem_mean_fields", "lbmdem_mean_fields_device", "lbmdem_mean_profile", "lbmdem_write_mean",
           "lbmdem_write_mean_files", "lbmdem_set_mean_output")
LX, LY = 6, 5


def planes(ux, uy, rho, diss, gdot, fluid, grain):
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (LX, LY)).copy()
    return dict(ux=full(ux), uy=full(uy), rho=full(rho), diss=full(diss), gdot=full(gdot), fluid=fluid, grain=grain)


def classes():
    """the inner nodes fluid, one grain's node, the outer ring a wall"""
    fluid = np.zeros((LX, LY), bool)
    fluid[1:-1, 1:-1] = True
    grain = np.zeros((LX, LY), bool)
    grain[2, 2] = True
    fluid[2, 2] = False
    return fluid, grain


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def chain_of(v, n):
    s = 0.0
    for _ in range(n):
        s = s + v
    return s


@pytest.mark.parametrize("n", [1, 2, 4, 5, 8, 16])
def test_a_constant_field_gives_the_chain_and_its_mean(n):
    fluid, grain = classes()
    rng = np.random.default_rng(n)
    if n in (1, 2, 4, 5):   # any doubles
        ux, uy, rho = rng.normal(0, 0.1, (LX, LY)), rng.normal(0, 0.1, (LX, LY)), rng.normal(1, 0.01, (LX, LY))
    else:                   # short significands: every partial sum and every product is exact
        ux, uy, rho = (rng.integers(-4096, 4096, (LX, LY)) / 4096. for _ in range(3))
    F = planes(ux, uy, rho, 0.375, 0.625, fluid, grain)
    acc = mu.window((LX, LY))
    for _ in range(n):
        mu.sample(acc, F)
    for name, v in (("Sux", ux), ("Suy", uy), ("Sxy", ux * uy), ("Srho2", rho * rho)):
        want = np.array([[chain_of(float(v[x, y]), n) if fluid[x, y] else 0.0 for y in range(LY)] for x in range(LX)])
        assert np.array_equal(bits(acc[name]), bits(want)), name
    want_g = np.where(grain, np.vectorize(lambda v: chain_of(float(v), n))(ux), 0.0)
    assert np.array_equal(bits(acc["Sgux"]), bits(want_g))
    assert np.array_equal(acc["n_fluid"], n * fluid) and np.array_equal(acc["n_grain"], n * grain)
    D = mu.derived(acc, n)
    assert np.array_equal(D["phi"], fluid.astype(float)) and np.array_equal(D["solid"], grain.astype(float))
    if n != 5:
        assert np.array_equal(bits(D["mux"]), bits(np.where(fluid, ux, 0.0))) and np.array_equal(bits(D["mrho"]), bits(np.where(fluid, rho, 0.0)))
        assert np.array_equal(bits(D["gux"]), bits(np.where(grain, ux, 0.0)))
        for name in ("rxx", "rxy", "ryy", "vrho"):
            assert np.array_equal(bits(D[name]), bits(np.zeros((LX, LY)))), name   # +0.0, the sign included
        assert np.array_equal(D["mdiss"], np.where(fluid, 0.375, 0.0)) and np.array_equal(D["mgdot"], np.where(fluid, 0.625, 0.0))
    else:   # five addends round: the mean is v to a few ulp, the variance zero to a few ulp of v * v
        assert np.allclose(D["mux"][fluid], ux[fluid], rtol=4 * 2.0 ** -52, atol=0)
        assert (np.abs(D["rxx"][fluid]) <= 8 * 2.0 ** -52 * (ux * ux)[fluid]).all()


def test_two_alternating_fields_give_the_mean_and_variance_computed_by_hand():
    """a = 0.5, b = 0.25 alternating, 6 samples: mean 0.375, variance ((0.25 + 0.0625) / 2) - 0.140625 = 0.015625 = ((a - b) / 2)^2;
    uy = -a, -b: ryy the same, rxy its negative; rho = 1 + a, 1 + b: vrho the same. Every number is a short binary fraction."""
    fluid, grain = classes()
    acc = mu.window((LX, LY))
    for k in range(6):
        v = (0.5, 0.25)[k % 2]
        mu.sample(acc, planes(v, -v, 1. + v, 2. * v, 4. * v, fluid, grain))
    D = mu.derived(acc, 6)
    z = lambda v: np.where(fluid, v, 0.0)
    assert np.array_equal(acc["Sux"], z(2.25)) and np.array_equal(acc["Sxx"], z(0.9375))
    assert np.array_equal(D["mux"], z(0.375)) and np.array_equal(D["muy"], z(-0.375)) and np.array_equal(D["mrho"], z(1.375))
    assert np.array_equal(D["rxx"], z(0.015625)) and np.array_equal(D["ryy"], z(0.015625)) and np.array_equal(D["rxy"], z(-0.015625))
    assert np.array_equal(D["vrho"], z(0.015625)) and np.array_equal(D["mdiss"], z(0.75)) and np.array_equal(D["mgdot"], z(1.5))
    assert np.array_equal(D["gux"], np.where(grain, 0.375, 0.0)) and np.array_equal(D["guy"], np.where(grain, -0.375, 0.0))
    P = mu.profile(D, acc["n_fluid"])
    assert P.shape == (14, LY)
    assert np.array_equal(P[2], 0.375 * fluid.sum(0)) and np.array_equal(P[13], 6. * fluid.sum(0)) and np.array_equal(P[0], 1. * fluid.sum(0))


def test_a_node_fluid_in_k_of_n_samples():
    """node (3, 3) is fluid in samples 0, 2, 3 of 5, a grain's in sample 1, a wall in sample 4: phi = 3 / 5, solid = 1 / 5, and its
    fluid planes hold the three fluid addends only, its grain planes the one"""
    fluid, grain = classes()
    vals = (0.1, 0.7, -0.3, 0.9, 5.0)
    acc = mu.window((LX, LY))
    for k, v in enumerate(vals):
        fl, gr = fluid.copy(), grain.copy()
        if k == 1:
            fl[3, 3], gr[3, 3] = False, True
        if k == 4:
            fl[3, 3] = False
        mu.sample(acc, planes(v, 2. * v, 1. + v, v, v, fl, gr))
    assert acc["n_fluid"][3, 3] == 3 and acc["n_grain"][3, 3] == 1 and acc["n_fluid"][1, 1] == 5 and acc["n_fluid"][0, 0] == 0
    assert acc["Sux"][3, 3] == ((0.0 + 0.1) + -0.3) + 0.9 and acc["Sgux"][3, 3] == 0.0 + 0.7 and acc["Sgux"][1, 1] == 0.0
    assert acc["Sxx"][3, 3] == ((0.0 + 0.1 * 0.1) + -0.3 * -0.3) + 0.9 * 0.9
    D = mu.derived(acc, 5)
    assert D["phi"][3, 3] == 3. / 5. and D["solid"][3, 3] == 1. / 5. and D["phi"][0, 0] == 0.0 and D["solid"][0, 0] == 0.0
    assert D["mux"][3, 3] == acc["Sux"][3, 3] / 3. and D["gux"][3, 3] == 0.7 and D["gux"][1, 1] == 0.0 and D["mux"][0, 0] == 0.0


def test_a_subset_window_leaves_the_other_fields_zero():
    fluid, grain = classes()
    acc = mu.window((LX, LY), mu.U | mu.GRAIN)
    assert sorted(acc) == sorted(["Sux", "Suy", "Sgux", "Sguy", "n_fluid", "n_grain"])
    mu.sample(acc, planes(0.5, 0.25, 1.0, 1.0, 1.0, fluid, grain))
    assert mu.available(acc) == ["phi", "solid", "mux", "muy", "gux", "guy"]
    D = mu.derived(acc, 1)
    assert D["mux"][1, 1] == 0.5 and not D["rxx"].any() and not D["mrho"].any() and D["guy"][2, 2] == 0.25
    assert mu.plane_names(mu.ALL) == [n for g in mu.PLANES for n in g] and mu.fmask_of(mu.FIELDS) == mu.FALL


def ragged():
    """seven planes 37 x 23 and a profile with a -0.0, a denormal and large values"""
    rng = np.random.default_rng(5)
    P = [rng.normal(0, 1, (37, 23)) for _ in range(7)]
    P[1][0, 0], P[1][36, 22], P[3][5, 7], P[6][1, 1] = -0.0, 1e-310, 1e300, -1e-310
    prof = rng.normal(0, 40, (14, 23))
    prof[2, 0], prof[3, 1], prof[4, 2], prof[5, 3] = -0.0, 1e-310, 37.0, -1e+100
    return P, prof


def test_write_mean_files_writes_the_documented_bytes(pkg, tmp_path):
    P, prof = ragged()
    pkg.write_mean_files(str(tmp_path), 7, 12345, *P, prof)
    assert sorted(os.listdir(tmp_path)) == ["mean000007.vtk", "mean_profile000007.dat"]
    assert (tmp_path / "mean000007.vtk").read_bytes() == mu.file_bytes(*P)
    text = (tmp_path / "mean_profile000007.dat").read_bytes()
    assert text == mu.profile_text(prof, 12345, 37)
    lines = text.decode().splitlines()
    assert lines[0] + "\n" == mu.PROFILE_HEADER and len(lines) == 24 and all(len(l.split()) == 15 for l in lines[1:])
    assert lines[1].split()[:2] == ["0", "12345"] and lines[1].split()[4] == "-0.000000e+00"
    assert lines[2].split()[5] == "%e" % (1e-310 / 37.0) and lines[3].split()[6] == "1.000000e+00"


def test_refusals_without_a_device(pkg, tmp_path):
    P, prof = ragged()
    with pytest.raises(pkg.LbmDemError, match="cannot open"):
        pkg.write_mean_files(str(tmp_path / "not" / "there"), 0, 1, *P, prof)
    with pytest.raises(pkg.LbmDemError, match="seven planes of one shape"):
        pkg.write_mean_files(str(tmp_path), 0, 1, *P[:6], P[6][:-1], prof)
    with pytest.raises(pkg.LbmDemError, match=r"a profile of shape \(14, ly\)"):
        pkg.write_mean_files(str(tmp_path), 0, 1, *P, prof[:13])
    with pytest.raises(pkg.LbmDemError, match="bad mask 32"):
        pkg.mean_plane_names(32)
    with pytest.raises(pkg.LbmDemError, match="bad field mask 0"):
        pkg.mean_field_names(0)
    L = pkg.load_library()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    d = os.fsencode(str(tmp_path))
    args = [vp(p) for p in P] + [vp(prof)]
    for k in range(8):
        bad = list(args)
        bad[k] = None
        assert L.lbmdem_write_mean_files(d, 0, 37, 23, 1, *bad) == -1 and L.lbmdem_last_error() == b"null buffer", k
    assert L.lbmdem_write_mean_files(None, 0, 37, 23, 1, *args) == -1 and L.lbmdem_last_error() == b"null directory"
    assert L.lbmdem_write_mean_files(d, 0, 1, 23, 1, *args) == -1 and L.lbmdem_write_mean_files(d, 0, 37, 1, 1, *args) == -1
    assert L.lbmdem_write_mean_files(d, 0, 37, 23, -1, *args) == -1 and b"-1 samples" in L.lbmdem_last_error()
    assert os.listdir(tmp_path) == []
    # no handle: refused before any device is looked for
    one = np.zeros(8)
    n = ctypes.c_long(0)
    for rc in (L.lbmdem_mean_begin(None, 31, 1), L.lbmdem_mean_sample(None), L.lbmdem_mean_reset(None), L.lbmdem_mean_end(None),
               L.lbmdem_mean_stats(None, vp(one)), L.lbmdem_mean_download(None, vp(one), vp(one), vp(one), 1, ctypes.byref(n)),
               L.lbmdem_mean_fields(None, 1, vp(one), 1, ctypes.byref(n)), L.lbmdem_mean_fields_device(None, 1, vp(one), 1),
               L.lbmdem_mean_profile(None, vp(one), 1), L.lbmdem_write_mean(None, d, 0), L.lbmdem_set_mean_output(None, 31, 1)):
        assert rc == -1 and b"null handle" in L.lbmdem_last_error()


def test_both_libraries_export_the_symbols(pkg, tmp_path):
    assert set(SYMBOLS) <= set(pkg.exported_symbols())
    L = pkg.load_library()
    assert all(hasattr(L, name) for name in SYMBOLS)
    assert os.path.exists(pkg.SP_LIB_PATH), "the single-precision library has not been built"
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    # the host-only writer works in the float library too; its device calls refuse a null handle as the double library's do
    P, prof = ragged()
    pkg.write_mean_files(str(tmp_path), 1, 3, *P, prof, precision="f32")
    assert (tmp_path / "mean000001.vtk").read_bytes() == mu.file_bytes(*P)
    assert (tmp_path / "mean_profile000001.dat").read_bytes() == mu.profile_text(prof, 3, 37)
    sp = pkg.load_library("f32")
    assert sp.lbmdem_mean_sample(None) == -1 and sp.lbmdem_set_mean_output(None, 31, 1) == -1
    # the package's constants are the restatement's
    assert (pkg.MEAN_U, pkg.MEAN_UU, pkg.MEAN_RHO, pkg.MEAN_DISS, pkg.MEAN_GRAIN, pkg.MEAN_ALL) == (mu.U, mu.UU, mu.RHO, mu.DISS, mu.GRAIN, mu.ALL)
    assert pkg.MEAN_PLANES == mu.PLANES and pkg.MEANF_NAMES == mu.FIELDS and pkg.MEANF_ALL == mu.FALL and pkg.MEANF_GUY == 4096
    assert pkg.MEAN_PROFILE_ROWS == mu.PROFILE_ROWS and pkg.mean_plane_names(mu.U | mu.GRAIN) == ["Sux", "Suy", "Sgux", "Sguy"]
    assert pkg.MEAN_COUNTERS == ("present", "mask", "samples", "hook_steps", "bytes")


def test_host_driver_knows_the_option(pkg):
    """`lbmdem --mean` is refused with --gpus N, with --dry and with a cadence of 0, before a file is read or a device looked for"""
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "host", "lbmdem")
    run = lambda *a: subprocess.run([exe, "no_such_sample.data", *a], capture_output=True, text=True)
    out = run("--mean", "--gpus", "2")
    assert out.returncode != 0 and "--mean is a single-GPU mode" in out.stderr
    out = run("--mean", "4", "--dry")
    assert out.returncode != 0 and "--mean cannot be combined with --dry" in out.stderr
    out = run("--mean", "0")
    assert out.returncode != 0 and "--mean [EVERY]" in out.stderr
    out = run("--no-such-option")
    assert "--mean [EVERY]" in out.stdout + out.stderr   # the usage line
