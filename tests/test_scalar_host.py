"""CPU: the passive scalar's specification -- the numpy restatement of tests/scalar_util.py -- pinned to physics that can be derived
(conservation in a closed box, the growth of the second moment, the drift of the centre of mass), and the host-only half of the
feature: lbmdem_write_scalar_files against bytes assembled here, scalar.data's line, the refusals that need no device, the
symbols of both libraries, the host driver's option. No device is touched.

What can be derived. With Ctot the total, m1 and m2 the first and second moment of C along one axis, J = sum_n sum_k e_k g_k(n)
and F = sum_n x J_x(n), one step (collide, then pull) on a lattice without boundaries gives, exactly,
    sum_n (g_1 + g_3) = Ctot / 3                     (it starts there -- g_k = w_k C -- and the collision keeps it there)
    J(t + 1) = (1 - omega) J(t) + omega Ctot u       m1(t + 1) - m1(t) = J(t + 1)
    F(t + 1) = (1 - omega) F(t) + Ctot / 3           m2(t + 1) - m2(t) = Ctot / 3 + 2 (1 - omega) F(t)      (u = 0)
with J(0) = F(0) = 0. For tau_s = 1 (omega = 1) the second moment grows by exactly 1/3 = 2 D and the centre of mass moves by
exactly u, from the first step on; for any other tau_s a transient (1 - omega)^t lies on top, which the recurrences give exactly,
and the growth tends to (2 - omega) / (3 omega) = 2 D. A population travels one node per step, so a point of dye 23 nodes from the
nearest wall is on an unbounded lattice for its first 22 steps: those are the steps compared."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import scalar_util as su

SYMBOLS = ("lbmdem_scalar_set", "lbmdem_scalar_step", "lbmdem_scalar_download", "lbmdem_scalar_download_state", "lbmdem_scalar_device",
           "lbmdem_scalar_sums", "lbmdem_scalar_stats", "lbmdem_write_scalar", "lbmdem_write_scalar_files", "lbmdem_set_scalar_output")
LX, LY = 64, 48
AT = (32, 24)       # the point of dye: 23 nodes from the nearest fluid node next to a wall
FREE_STEPS = 22     # ... so nothing has met a wall during the first 22 steps
U = 2.0 ** -53      # unit roundoff
# Largest deviation of the restatement from the recurrences above over the compared steps, measured on the CPU (LABBOOK.md); the
# moments are evaluated with math.fsum, so these figures are the roundings of the steps and of C * x. The tests allow four times
# them, and never more than 1 % of 2 D or of |u|.
MEASURED_M2 = {1.0: 1.5e-15, 0.8: 6.2e-16}
MEASURED_M1 = {1.0: 4.3e-15, 0.8: 7.2e-15}


def box():
    """a closed box without grains: fluid inside, the lattice-edge walls around it (any owner but -1)"""
    obst = np.zeros((LX, LY), np.int32)
    obst[1:-1, 1:-1] = -1
    return obst


def moments(g):
    """-> (total, centre x, centre y, second moment about the centre along x, along y), the sums exact (math.fsum)"""
    C = su.conc(g)
    xs = np.arange(LX, dtype=np.float64)[:, None] * np.ones((1, LY))
    ys = np.ones((LX, 1)) * np.arange(LY, dtype=np.float64)[None, :]
    tot = math.fsum(C.ravel())
    mx, my = math.fsum((C * xs).ravel()) / tot, math.fsum((C * ys).ravel()) / tot
    vx, vy = math.fsum((C * (xs - mx) ** 2).ravel()) / tot, math.fsum((C * (ys - my) ** 2).ravel()) / tot
    return tot, mx, my, vx, vy


def point():
    C = np.zeros((LX, LY))
    C[AT] = 1.0
    return su.initial(C, box())


@pytest.mark.parametrize("tau", [1.0, 0.8])
def test_closed_box_conserves_and_spreads_by_2D_per_step(tau):
    omega, D = 1. / tau, su.diffusivity(tau)
    obst = box()
    g, was = point()
    rest = np.zeros((LX, LY))
    total0 = math.fsum(g.ravel())
    prev = moments(g)
    F, dev, late, largest = 0.0, 0.0, 0.0, 0.0
    for t in range(60):
        g, was = su.step(g, was, obst, rest, rest, omega)
        largest = max(largest, math.fsum(np.abs(g).ravel()))
        now = moments(g)
        if t < FREE_STEPS:
            want = 1. / 3 + 2. * (1. - omega) * F
            dev = max(dev, abs(now[3] - prev[3] - want), abs(now[4] - prev[4] - want))
            if t >= FREE_STEPS - 4:
                late = max(late, abs(now[3] - prev[3] - 2. * D), abs(now[4] - prev[4] - 2. * D))
        F = (1. - omega) * F + 1. / 3
        prev = now
    # Conservation. Per step a population is touched by: the four additions of C, w_k * C, the bracket's product, g_k - eq_k,
    # the product with omega, the final subtraction -- 9 roundings, each at most U relative to a value that is at most the sum
    # of the |g_k| of its node; the pull and the bounce-back copy. So the total moves by at most 9 U sum |g| per step.
    drift = abs(math.fsum(g.ravel()) - total0)
    bound = 60 * 9 * U * largest
    print(f"tau_s {tau}: total drift {drift:.3e} (bound {bound:.3e}), second moment vs recurrence {dev:.3e}, "
          f"last free steps vs 2 D = {2 * D:.6f}: {late:.3e}")
    assert drift <= bound
    assert (su.conc(g)[~was] == 0.0).all() and np.array_equal(was, obst == -1)
    # the second moment, both axes
    assert dev <= 4 * MEASURED_M2[tau] and dev < 0.01 * 2 * D
    # ... and it has settled on 2 D: the transient left is (1 - omega)^t, t >= 18
    assert late <= 2. / 3 * abs(1. - omega) ** (FREE_STEPS - 4) / omega + 4 * MEASURED_M2[tau]
    assert late < 0.01 * 2 * D


@pytest.mark.parametrize("tau", [1.0, 0.8])
def test_uniform_velocity_carries_the_centre_of_mass(tau):
    """u the same at every node: 20 steps, the patch (20 nodes of reach at most) stays clear of the walls"""
    omega = 1. / tau
    u = (0.05, -0.03)
    obst = box()
    g, was = point()
    ux, uy = np.full((LX, LY), u[0]), np.full((LX, LY), u[1])
    prev = moments(g)
    dev = 0.0
    for t in range(20):
        g, was = su.step(g, was, obst, ux, uy, omega)
        now = moments(g)
        settled = 1. - (1. - omega) ** (t + 1)   # J(t + 1) / (Ctot u)
        dev = max(dev, abs(now[1] - prev[1] - u[0] * settled), abs(now[2] - prev[2] - u[1] * settled))
        prev = now
    C = su.conc(g)
    assert (C[:AT[0] - 20] == 0).all() and (C[AT[0] + 21:] == 0).all() and (C[:, :AT[1] - 20] == 0).all() and (C[:, AT[1] + 21:] == 0).all()
    print(f"tau_s {tau}: centre of mass vs u per step {dev:.3e}")
    assert dev <= 4 * MEASURED_M1[tau] and dev < 0.01 * min(abs(u[0]), abs(u[1]))
    if tau == 1.0:   # no transient: the centre has moved by 20 u
        assert abs(now[1] - AT[0] - 20 * u[0]) <= 20 * 4 * MEASURED_M1[tau] and abs(now[2] - AT[1] - 20 * u[1]) <= 20 * 4 * MEASURED_M1[tau]


def test_refill_and_bounce_back_by_hand():
    """a 5 x 5 box, scalar loops over the header's rules: a node uncovered between two steps takes the mean of its eligible
    neighbours, a covered node is emptied, and nothing crosses a solid node"""
    obst = np.zeros((5, 5), np.int32)
    obst[1:-1, 1:-1] = -1
    obst[2, 2] = 0                       # a one-node grain
    rng = np.random.default_rng(5)
    C = rng.uniform(0.5, 1.5, (5, 5))
    g, was = su.initial(C, obst)
    assert not was[2, 2] and (g[2, 2] == 0).all() and was[1, 1]
    obst2 = obst.copy()
    obst2[2, 2] = -1                     # uncovered ...
    obst2[1, 1] = 0                      # ... and (1, 1) covered
    filled, cnt = su.refill(g, was, obst2)
    stored = su.conc(g)
    # (2, 2): neighbours in the order q = 2, 4, 6, 8 = (1, 2), (2, 1), (3, 2), (2, 3), all fluid and held
    Cf = (((0.0 + stored[1, 2]) + stored[2, 1]) + stored[3, 2]) + stored[2, 3]
    Cf = Cf / 4.0
    assert cnt[2, 2] == 4 and np.array_equal(filled[2, 2], [w * Cf for w in su.W])
    assert (cnt[obst2 != -1] == -1).all() and cnt[3, 3] == -1
    ux, uy = rng.normal(0, 0.05, (5, 5)), rng.normal(0, 0.05, (5, 5))
    omega = 1. / 0.7
    g2, was2 = su.step(g, was, obst2, ux, uy, omega)
    assert (g2[1, 1] == 0).all() and not was2[1, 1] and was2[2, 2]
    # node (1, 2) by hand: its -x neighbour (0, 2) is a wall, its -y neighbour (1, 1) is now solid
    def star(x, y):
        gg = filled[x, y]
        Cn = (((gg[0] + gg[1]) + gg[2]) + gg[3]) + gg[4]
        s = (0.0, -ux[x, y], -uy[x, y], ux[x, y], uy[x, y])
        eq = [su.W[0] * Cn] + [(su.W[k] * Cn) * (1. + (3. * s[k])) for k in range(1, 5)]
        return [gg[k] - (omega * (gg[k] - eq[k])) for k in range(5)]
    own = star(1, 2)
    want = [own[0], star(2, 2)[1], star(1, 3)[2], own[1], own[2]]   # k = 3 from (0, 2): wall -> own opp = 1; k = 4 from (1, 1): solid -> own 2
    assert np.array_equal(g2[1, 2], want)


def test_sums_restatement_is_the_chain():
    rng = np.random.default_rng(9)
    lx, ly = 7, 150
    g = rng.normal(0, 1, (lx, ly, 5))
    was = rng.random((lx, ly)) < 0.7
    g[~was] = 0.0
    s = su.sums(g, was)
    C = su.conc(g)
    rows = []
    for x in range(lx):
        blocks = []
        for b in range(0, ly, 64):
            a = a2 = 0.0
            for y in range(b, min(ly, b + 64)):
                a = a + (C[x, y] if was[x, y] else 0.0)
                a2 = a2 + (C[x, y] * C[x, y] if was[x, y] else 0.0)
            blocks.append((a, a2))
        r = r2 = 0.0
        for a, a2 in blocks:
            r, r2 = r + a, r2 + a2
        rows.append((r, r2))
    t = t2 = 0.0
    for r, r2 in rows:
        t, t2 = t + r, t2 + r2
    assert s == dict(n_fluid=float(was.sum()), sum_C=t, sum_C2=t2, min_C=C[was].min(), max_C=C[was].max())
    assert su.sums(np.zeros((3, 3, 5)), np.zeros((3, 3), bool)) == dict(n_fluid=0.0, sum_C=0.0, sum_C2=0.0, min_C=0.0, max_C=0.0)


def _plane(lx=37, ly=23, seed=3):
    """values float cannot hold exactly, a negative zero, one beyond its range"""
    C = np.random.default_rng(seed).normal(0.0, 1.0, (lx, ly))
    C[1, 0] = -0.0
    C[2, 1] = 1.0 / 3.0
    C[3, 0] = 1.0e+60   # -> +inf as a float
    return C


def test_file_is_exactly_the_expected_bytes(pkg, tmp_path):
    C = _plane()
    lx, ly = C.shape
    pkg.write_scalar_files(str(tmp_path), 7, C)
    got = (tmp_path / "scalar000007.vtk").read_bytes()
    assert os.listdir(tmp_path) == ["scalar000007.vtk"]
    # assembled here, independently of scalar_util.file_bytes
    head = b"# vtk DataFile Version 2.0\nlbmdem passive scalar\nBINARY\nDATASET STRUCTURED_POINTS\n"
    head += b"DIMENSIONS 37 23 1\nORIGIN 0 0 0\nSPACING 0.0270270277 0.0270270277 1\n"
    head += b"POINT_DATA 851\nSCALARS concentration float\nLOOKUP_TABLE default\n"
    assert b"%.9g" % float(np.float32(1. / 37)) == b"0.0270270277"
    assert got[:len(head)] == head
    with np.errstate(over="ignore"):
        body = np.array([C[x, y] for y in range(ly) for x in range(lx)]).astype(np.float32).astype(">f4").tobytes()
    assert got[len(head):] == body and got == su.file_bytes(C)
    assert np.isinf(np.frombuffer(body, ">f4").reshape(ly, lx)[0, 3])


def test_scalar_data_line():
    """scalar.data's line is %le of the step counter and of the five sums (C's "%le" is Python's "%e")"""
    s = dict(n_fluid=1234.0, sum_C=1.0 / 3.0, sum_C2=2.5e-7, min_C=-0.0, max_C=1.0e+100)
    assert su.data_line(4000, s) == "4.000000e+03 1.234000e+03 3.333333e-01 2.500000e-07 -0.000000e+00 1.000000e+100\n"
    assert su.DATA_HEADER == "# step n_fluid sum_C sum_C2 min_C max_C\n"


def test_refusals_without_a_device(pkg, tmp_path):
    C = _plane()
    with pytest.raises(pkg.LbmDemError, match="cannot open"):
        pkg.write_scalar_files(str(tmp_path / "not" / "there"), 0, C)
    with pytest.raises(pkg.LbmDemError, match=r"\(lx, ly\)"):
        pkg.write_scalar_files(str(tmp_path), 0, C.ravel())
    L = pkg.load_library()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    d = os.fsencode(str(tmp_path))
    assert L.lbmdem_write_scalar_files(d, 0, 37, 23, None) == -1 and b"null buffer" in L.lbmdem_last_error()
    assert L.lbmdem_write_scalar_files(None, 0, 37, 23, vp(C)) == -1 and b"null directory" in L.lbmdem_last_error()
    assert L.lbmdem_write_scalar_files(d, 0, 1, 23, vp(C)) == -1 and L.lbmdem_write_scalar_files(d, 0, 37, 1, vp(C)) == -1
    assert os.listdir(tmp_path) == []
    # no handle: refused before any device is looked for
    p = ctypes.c_void_p()
    assert L.lbmdem_scalar_set(None, vp(C), 1.0, 1) == -1
    assert L.lbmdem_scalar_step(None) == -1
    assert L.lbmdem_scalar_download(None, vp(C)) == -1
    assert L.lbmdem_scalar_download_state(None, vp(C), vp(C)) == -1
    assert L.lbmdem_scalar_device(None, ctypes.byref(p), 1) == -1
    assert L.lbmdem_scalar_sums(None, vp(np.zeros(5))) == -1
    assert L.lbmdem_scalar_stats(None, vp(np.zeros(3, np.int64))) == -1
    assert L.lbmdem_write_scalar(None, d, 0) == -1
    assert L.lbmdem_set_scalar_output(None, 1) == -1
    assert b"null handle" in L.lbmdem_last_error()


def test_both_libraries_export_the_symbols(pkg, tmp_path):
    assert set(SYMBOLS) <= set(pkg.exported_symbols())
    L = pkg.load_library()
    assert all(hasattr(L, name) for name in pkg.exported_symbols())
    assert os.path.exists(pkg.SP_LIB_PATH), "the single-precision library has not been built"
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    # the host-only writer works in the float library too; its device calls refuse a null handle as the double library's do
    C = _plane()
    pkg.write_scalar_files(str(tmp_path), 1, C, precision="f32")
    assert (tmp_path / "scalar000001.vtk").read_bytes() == su.file_bytes(C)
    sp = pkg.load_library("f32")
    assert sp.lbmdem_scalar_step(None) == -1 and sp.lbmdem_set_scalar_output(None, 1) == -1
    assert pkg.SCALAR_SUMS == su.SUMS and pkg.SCALAR_COUNTERS == ("present", "steps", "hook_steps")


def test_host_driver_knows_the_option(pkg):
    """`lbmdem --dye` is refused with --gpus N, with --dry and without a box, before a file is read or a device looked for"""
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "host", "lbmdem")
    run = lambda *a: subprocess.run([exe, "no_such_sample.data", *a], capture_output=True, text=True)
    out = run("--dye", "1,1,8,8", "--gpus", "2")
    assert out.returncode != 0 and "--dye is a single-GPU mode" in out.stderr
    out = run("--dye", "1,1,8,8", "--dry")
    assert out.returncode != 0 and "--dye cannot be combined with --dry" in out.stderr
    for bad in ("8", "1,1,8", "4,4,2,8", "1,1,8,8x", "-1,0,3,3"):
        out = run("--dye", bad)
        assert out.returncode != 0 and "--dye X0,Y0,X1,Y1" in out.stderr, bad
    for bad in ("0.5", "nan", "x"):
        out = run("--dye", "1,1,8,8", "--dye-tau", bad)
        assert out.returncode != 0 and "--dye-tau T" in out.stderr, bad
