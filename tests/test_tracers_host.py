"""CPU: the host-only half of the fluid tracers (include/lbmdem_hip.h) -- lbmdem_write_tracers_files against bytes assembled in
tests/tracer_util.py, the refusals that need no device, the symbols of both libraries, the host driver's option -- and the numpy
restatement of the advance against the same arithmetic written as scalar loops. No device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tracer_util as tu

SYMBOLS = ("lbmdem_tracer_set", "lbmdem_tracer_advance", "lbmdem_tracer_download", "lbmdem_tracer_device", "lbmdem_tracer_sample",
           "lbmdem_tracer_stats", "lbmdem_write_tracers", "lbmdem_write_tracers_files", "lbmdem_set_tracer_output")
LX, LY = 37, 23


def _set(n, seed=3):
    """n positions inside the domain and a sample with values float cannot hold exactly, a negative zero, one beyond its range"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 1.0, (n, 2)) * (LX - 1, LY - 1)
    uvo = np.empty((n, 3))
    uvo[:, :2] = rng.normal(0.0, 0.05, (n, 2))
    uvo[:, 2] = rng.integers(-1, 7, n)
    if n > 3:
        uvo[1, 0] = -0.0
        uvo[2, 1] = 1.0 / 3.0
        uvo[3, 0] = 1.0e+60   # -> +inf as a float
    return xy, uvo


@pytest.mark.parametrize("n", [0, 1, 300])
def test_file_is_exactly_the_expected_bytes(pkg, tmp_path, n):
    xy, uvo = _set(n)
    pkg.write_tracers_files(str(tmp_path), 7, LX, xy, uvo)
    got = (tmp_path / "tracers000007.vtk").read_bytes()
    assert got == tu.file_bytes(LX, xy, uvo)
    assert os.listdir(tmp_path) == ["tracers000007.vtk"]
    # the layout, piece by piece
    head = b"# vtk DataFile Version 2.0\nlbmdem fluid tracers\nBINARY\nDATASET POLYDATA\nPOINTS %d float\n" % n
    assert got.startswith(head)
    at = len(head)
    pts = np.frombuffer(got, ">f4", 3 * n, at).reshape(n, 3)
    pas = np.float32(1.0 / LX)
    assert np.array_equal(pts[:, 0], xy[:, 0].astype(np.float32) * pas) and np.array_equal(pts[:, 1], xy[:, 1].astype(np.float32) * pas)
    assert not pts[:, 2].any()
    at += 12 * n
    line = b"VERTICES %d %d\n" % (n, 2 * n)
    assert got[at:at + len(line)] == line
    at += len(line)
    cells = np.frombuffer(got, ">i4", 2 * n, at).reshape(n, 2)
    assert (cells[:, 0] == 1).all() and np.array_equal(cells[:, 1], np.arange(n))
    at += 8 * n
    line = b"POINT_DATA %d\nVECTORS tracer_velocity_lb float\n" % n
    assert got[at:at + len(line)] == line
    at += len(line)
    with np.errstate(over="ignore"):
        vec = np.frombuffer(got, ">f4", 3 * n, at).reshape(n, 3)
        assert np.array_equal(vec[:, :2], uvo[:, :2].astype(np.float32)) and not vec[:, 2].any()
        at += 12 * n
        line = b"SCALARS tracer_owner float\nLOOKUP_TABLE default\n"
        assert got[at:at + len(line)] == line
        at += len(line)
        assert np.array_equal(np.frombuffer(got, ">f4", n, at), uvo[:, 2].astype(np.float32))
    assert at + 4 * n == len(got)
    if n > 3:
        assert vec[3, 0] == np.inf and np.signbit(vec[1, 0])


def test_domain_corners_land_on_the_mesh_corners(pkg, tmp_path):
    """the four corners of the domain: 0 and (float)(l - 1) * (float)(1 / lx), the last coordinates of the frames' mesh"""
    xy = np.array([[0.0, 0.0], [LX - 1.0, 0.0], [0.0, LY - 1.0], [LX - 1.0, LY - 1.0]])
    uvo = np.zeros((4, 3))
    uvo[:, 2] = 5.0   # (a corner's nearest node is a lattice-edge wall: the owner is nbgrains)
    pkg.write_tracers_files(str(tmp_path), 0, LX, xy, uvo)
    got = (tmp_path / "tracers000000.vtk").read_bytes()
    assert got == tu.file_bytes(LX, xy, uvo)
    at = got.index(b"POINTS 4 float\n") + len(b"POINTS 4 float\n")
    pts = np.frombuffer(got, ">f4", 12, at).reshape(4, 3)
    pas = np.float32(1.0 / LX)
    mesh_x, mesh_y = np.arange(LX, dtype=np.float32) * pas, np.arange(LY, dtype=np.float32) * pas   # (flow_util.file_bytes)
    assert np.array_equal(pts[:, 0], [mesh_x[0], mesh_x[-1], mesh_x[0], mesh_x[-1]])
    assert np.array_equal(pts[:, 1], [mesh_y[0], mesh_y[0], mesh_y[-1], mesh_y[-1]])


def test_missing_directory_and_bad_arguments_are_refused(pkg, tmp_path):
    xy, uvo = _set(5)
    with pytest.raises(pkg.LbmDemError, match="cannot open") as e:
        pkg.write_tracers_files(str(tmp_path / "not" / "there"), 0, LX, xy, uvo)
    assert e.value.code == -1
    with pytest.raises(pkg.LbmDemError, match="write_tracers_files"):
        pkg.write_tracers_files(str(tmp_path), 0, LX, xy, uvo[:4])
    L = pkg.load_library()
    d = str(tmp_path).encode()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.lbmdem_write_tracers_files(d, 0, LX, 5, None, vp(uvo)) == -1
    assert L.lbmdem_write_tracers_files(d, 0, LX, 5, vp(xy), None) == -1
    assert L.lbmdem_write_tracers_files(d, 0, LX, -1, vp(xy), vp(uvo)) == -1
    assert L.lbmdem_write_tracers_files(d, 0, 1, 5, vp(xy), vp(uvo)) == -1
    assert os.listdir(tmp_path) == []
    # no handle: refused before any device is looked for
    cnt = ctypes.c_long(0)
    p = ctypes.c_void_p()
    assert L.lbmdem_tracer_set(None, 5, vp(xy), 1) == -1
    assert L.lbmdem_tracer_advance(None) == -1
    assert L.lbmdem_tracer_download(None, None, 0, ctypes.byref(cnt)) == -1
    assert L.lbmdem_tracer_device(None, ctypes.byref(p)) == -1
    assert L.lbmdem_tracer_sample(None, None, 0, ctypes.byref(cnt)) == -1
    assert L.lbmdem_tracer_stats(None, vp(np.zeros(3, np.int64))) == -1
    assert L.lbmdem_write_tracers(None, d, 0) == -1
    assert L.lbmdem_set_tracer_output(None, 1) == -1
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
    xy, uvo = _set(300)
    pkg.write_tracers_files(str(tmp_path), 1, LX, xy, uvo, precision="f32")
    assert (tmp_path / "tracers000001.vtk").read_bytes() == tu.file_bytes(LX, xy, uvo)
    sp = pkg.load_library("f32")
    assert sp.lbmdem_tracer_advance(None) == -1 and sp.lbmdem_set_tracer_output(None, 1) == -1
    assert pkg.TRACER_COUNTERS == ("tracers", "advances", "hook_advances")


def test_host_driver_knows_the_option(pkg):
    """`lbmdem --tracers` is refused with --gpus N, with --dry and without a grid, before a file is read or a device looked for"""
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "host", "lbmdem")
    run = lambda *a: subprocess.run([exe, "no_such_sample.data", *a], capture_output=True, text=True)
    out = run("--tracers", "8x8", "--gpus", "2")
    assert out.returncode != 0 and "--tracers is a single-GPU mode" in out.stderr
    out = run("--tracers", "8x8", "--dry")
    assert out.returncode != 0 and "--tracers cannot be combined with --dry" in out.stderr
    for bad in ("8", "0x4", "8x8x"):
        out = run("--tracers", bad)
        assert out.returncode != 0 and "--tracers NXxNY" in out.stderr, bad


def _scalar_advance(ux, uy, px, py):
    """the header's advance for one tracer, Python floats (IEEE doubles), one operation at a time"""
    lx, ly = ux.shape

    def clamp(v, last):
        return 0.0 if not (v >= 0.0) else (float(last) if v > float(last) else v)

    def vel(px, py):
        i, j = min(int(px), lx - 2), min(int(py), ly - 2)
        a, b = px - i, py - j
        w00, w10, w01, w11 = (1. - a) * (1. - b), a * (1. - b), (1. - a) * b, a * b
        U = (((w00 * ux[i, j]) + (w10 * ux[i + 1, j])) + (w01 * ux[i, j + 1])) + (w11 * ux[i + 1, j + 1])
        V = (((w00 * uy[i, j]) + (w10 * uy[i + 1, j])) + (w01 * uy[i, j + 1])) + (w11 * uy[i + 1, j + 1])
        return U, V

    U0, V0 = vel(px, py)
    qx, qy = clamp(px + 0.5 * U0, lx - 1), clamp(py + 0.5 * V0, ly - 1)
    U1, V1 = vel(qx, qy)
    return clamp(px + U1, lx - 1), clamp(py + V1, ly - 1)


def test_restatement_is_the_header_written_as_a_loop():
    """tracer_util.advance against scalar loops on planes with every kind of value: ordinary, huge (the clamp on both sides), a NaN
    and an infinity (-> coordinate 0), tracers on nodes, on the corners and a hair inside the last node"""
    rng = np.random.default_rng(11)
    ux = rng.normal(0.0, 0.8, (LX, LY))
    uy = rng.normal(0.0, 0.8, (LX, LY))
    ux[5, 5], uy[9, 4], ux[30, 20], uy[12, 12] = 1.0e3, -1.0e3, np.nan, np.inf
    xy = rng.uniform(0.0, 1.0, (400, 2)) * (LX - 1, LY - 1)
    xy[:6] = [[0, 0], [LX - 1, 0], [0, LY - 1], [LX - 1, LY - 1], [LX - 1 - 1e-12, 3.0], [29.5, 19.5]]
    xy[6:12] = np.floor(xy[6:12])
    for _ in range(3):
        with np.errstate(all="ignore"):
            want = np.array([_scalar_advance(ux, uy, float(p[0]), float(p[1])) for p in xy])
        got = tu.advance(ux, uy, xy)
        assert tu.same(got, want)
        assert (got >= 0).all() and (got[:, 0] <= LX - 1).all() and (got[:, 1] <= LY - 1).all()
        xy = got
    assert (xy == 0).any() and (xy[:, 0] == LX - 1).any() and (xy[:, 1] == LY - 1).any()
    s = tu.sample(ux, uy, np.full((LX, LY), -1, np.int32), xy)
    assert s.shape == (400, 3) and (s[:, 2] == -1).all()
    g = tu.grid_seeds(LX, LY, 4, 3)
    assert g.shape == (12, 2) and g[0, 0] == 0.5 * (LX - 1) / 4 and g[1, 1] == 1.5 * (LY - 1) / 3 and g[3, 0] == 1.5 * (LX - 1) / 4
