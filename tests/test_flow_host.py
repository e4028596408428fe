"""CPU: the host-only half of the flow fields (include/lbmdem_hip.h) -- lbmdem_write_flow_files against bytes assembled here, the
mask and plane arithmetic, the refusals that need no device, the symbols of both libraries -- and a physical check of the
definition of the strain rate on the CPU oracle. No device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import flow_util as fu

SYMBOLS = ("lbmdem_flow_fields", "lbmdem_flow_fields_device", "lbmdem_flow_sums", "lbmdem_write_flow", "lbmdem_write_flow_files",
           "lbmdem_set_flow_output")


def _planes(lx=5, ly=3):
    """five planes, every value different, with negatives, zeros, a value float cannot hold exactly and one beyond its range"""
    p = [((np.arange(lx * ly).reshape(lx, ly) + 1) * (k + 1) * 1.1e-3) * (-1) ** k for k in range(5)]
    p[0][1, 2] = 0.0
    p[2][3, 1] = -0.0
    p[3][4, 0] = 1.0 / 3.0
    p[4][0, 0] = 1.0e+60   # -> +inf as a float
    return p


def test_constants_match_the_header(pkg):
    header = open(pkg.HEADER_PATH).read()
    for k, name in enumerate(fu.NAMES):
        assert f"#define LBMDEM_FLOW_{name.upper()} {1 << k}\n" in header
        assert getattr(pkg, f"FLOW_{name.upper()}") == 1 << k
    assert "#define LBMDEM_FLOW_ALL 255\n" in header and pkg.FLOW_ALL == fu.ALL == 255
    assert pkg.FLOW_NAMES == fu.NAMES and pkg.FLOW_SUMS == fu.SUMS


@pytest.mark.parametrize("mask,want", [(255, list(fu.NAMES)), (1, ["ux"]), (128, ["diss"]), (4 | 64, ["vort", "gdot"]),
                                       (2 | 8 | 32, ["uy", "div", "nxy"]), (1 | 2 | 4 | 64 | 128, ["ux", "uy", "vort", "gdot", "diss"])])
def test_plane_order_is_bit_order(pkg, mask, want):
    assert pkg.flow_plane_names(mask) == want == fu.plane_names(mask)


def test_bad_masks_are_refused(pkg):
    for mask in (0, 256, -1, 511, 1 << 20):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.flow_plane_names(mask)
        assert e.value.code == -1


def test_file_is_exactly_the_expected_bytes(pkg, tmp_path):
    p = _planes()
    with np.errstate(over="ignore"):
        want = fu.file_bytes(*p)
    pkg.write_flow_files(str(tmp_path), 7, *p)
    got = (tmp_path / "flow000007.vtk").read_bytes()
    assert got == want
    assert sorted(os.listdir(tmp_path)) == ["flow000007.vtk"]
    # the mesh and header conventions of the files lbmdem_write_vtk_fields writes: everything in front of the first variable
    fields11 = np.zeros(11 * 15, np.float32)
    pkg.write_vtk_fields(str(tmp_path), 7, 5, 3, fields11)
    frame = (tmp_path / "fluid_velocity_000007.vtk").read_bytes()
    head = frame[:frame.index(b"VECTORS")]
    assert head.endswith(b"POINT_DATA 15\n") and got.startswith(head + b"VECTORS fluid_velocity_lb float\n")
    # payloads: x fastest, big-endian float, the vector's third component 0
    at = len(head) + len(b"VECTORS fluid_velocity_lb float\n")
    vec = np.frombuffer(got, ">f4", 45, at).reshape(3, 5, 3)
    assert np.array_equal(vec[:, :, 0], p[0].T.astype(np.float32)) and np.array_equal(vec[:, :, 1], p[1].T.astype(np.float32))
    assert not vec[:, :, 2].any()
    at += 45 * 4
    with np.errstate(over="ignore"):
        for name, q in (("vorticity", p[2]), ("shear_rate", p[3]), ("dissipation", p[4])):
            line = b"SCALARS %s float\nLOOKUP_TABLE default\n" % name.encode()
            assert got[at:at + len(line)] == line
            at += len(line)
            assert np.array_equal(np.frombuffer(got, ">f4", 15, at).reshape(3, 5), q.T.astype(np.float32))
            at += 60
    assert at == len(got)
    assert np.frombuffer(got, ">f4", 1, at - 60)[0] == np.inf   # the double beyond float's range


def test_missing_directory_and_bad_arguments_are_refused(pkg, tmp_path):
    p = _planes()
    with pytest.raises(pkg.LbmDemError, match="cannot open") as e:
        pkg.write_flow_files(str(tmp_path / "not" / "there"), 0, *p)
    assert e.value.code == -1
    with pytest.raises(pkg.LbmDemError, match="one shape"):
        pkg.write_flow_files(str(tmp_path), 0, p[0], p[1], p[2], p[3], p[4][:4])
    L = pkg.load_library()
    d = str(tmp_path).encode()
    vp = [q.ctypes.data_as(ctypes.c_void_p) for q in p]
    for k in range(5):
        args = list(vp)
        args[k] = None
        assert L.lbmdem_write_flow_files(d, 0, 5, 3, *args) == -1
    assert L.lbmdem_write_flow_files(d, 0, 1, 3, *vp) == -1
    assert L.lbmdem_write_flow_files(d, 0, 5, 1, *vp) == -1
    assert os.listdir(tmp_path) == []
    # no handle: refused before any device is looked for
    cnt = ctypes.c_long(0)
    out = np.zeros(8)
    assert L.lbmdem_flow_fields(None, 255, None, 0, ctypes.byref(cnt)) == -1
    assert L.lbmdem_flow_fields_device(None, 255, None, 0) == -1
    assert L.lbmdem_flow_sums(None, out.ctypes.data_as(ctypes.c_void_p)) == -1
    assert L.lbmdem_write_flow(None, d, 0) == -1
    assert L.lbmdem_set_flow_output(None, 1) == -1


def test_both_libraries_export_the_symbols(pkg, tmp_path):
    assert set(SYMBOLS) <= set(pkg.exported_symbols())
    assert os.path.exists(pkg.SP_LIB_PATH), "the single-precision library has not been built"
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    # the host-only writer works in the float library too; its device calls refuse a null handle as the double library's do
    p = _planes()
    pkg.write_flow_files(str(tmp_path), 1, *p, precision="f32")
    with np.errstate(over="ignore"):
        assert (tmp_path / "flow000001.vtk").read_bytes() == fu.file_bytes(*p)
    sp = pkg.load_library("f32")
    assert sp.lbmdem_flow_sums(None, None) == -1 and sp.lbmdem_set_flow_output(None, 1) == -1


def test_host_driver_knows_the_option(pkg):
    """`lbmdem --flow` is refused with --gpus N and with --dry, before a file is read or a device looked for"""
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "host", "lbmdem")
    run = lambda *a: subprocess.run([exe, "no_such_sample.data", *a], capture_output=True, text=True)
    out = run("--flow", "--gpus", "2")
    assert out.returncode != 0 and "--flow is a single-GPU mode" in out.stderr
    out = run("--flow", "--dry")
    assert out.returncode != 0 and "--flow cannot be combined with --dry" in out.stderr


def test_three_level_chain_is_what_a_serial_loop_adds():
    """flow_util.total against the header's order of additions written as loops (a last block of 57 columns)"""
    rng = np.random.default_rng(5)
    v = rng.uniform(0.0, 1.0, (7, 121)) * 10.0 ** rng.integers(-8, 8, (7, 121))
    rows = []
    for x in range(7):
        blocks = []
        for b in range(2):
            a = 0.0
            for y in range(b * 64, min(121, b * 64 + 64)):
                a = a + v[x, y]
            blocks.append(a)
        a = 0.0
        for s in blocks:
            a = a + s
        rows.append(a)
    a = 0.0
    for s in rows:
        a = a + s
    assert fu.total(v) == a


def test_strain_rate_from_the_moments_is_the_velocity_gradient(pkg, po):
    """The definition, on the oracle: a lid-driven channel (set_lid) 64 x 40 with one small grain in a corner, s8 = s9 = 1 so
    that 3000 fluid steps reach the steady profile (nu = 1/6; at the default 1.9841, nu = 0.0013, the cavity is at Re ~ 600 and
    never steady: its acoustic transients over-relax and say nothing about the definition). In the grain-free middle, three nodes
    from the plates, T of the moments agrees with the central difference d(uy)/dx + d(ux)/dy of the same state."""
    lx, ly = 64, 40
    phys = pkg.Physics()
    pkg.load_library().lbmdem_physics_defaults(ctypes.byref(phys))
    phys.s8 = phys.s9 = 1.0
    o = po.Oracle(lx, ly, np.array([0.3e-3]), np.array([0.6e-3]), np.array([0.6e-3]))
    o.set_physics(np.array([getattr(phys, n) for n, _ in pkg.Physics._fields_[:29]]), phys.updateVerlet, phys.stepFilm)
    o.set_lid(0.05)
    o.lbm_steps(3000)
    sc = o.scalars()
    F = fu.fields(o.get_f(), o.get_obst(), o.get_grains()[:, :9], sc["Mgx"], sc["Mby"], sc["dx"], sc["c"], phys.s8, phys.s9, 1)
    ux, uy = F["ux"], F["uy"]
    cd = np.zeros_like(ux)
    cd[1:-1, 1:-1] = (uy[2:, 1:-1] - uy[:-2, 1:-1]) * 0.5 + (ux[1:-1, 2:] - ux[1:-1, :-2]) * 0.5
    reg = (slice(lx // 2 - 8, lx // 2 + 8), slice(3, ly - 3))
    assert F["fluid"][reg].all()
    scale = np.abs(cd[reg]).max()
    dev = np.abs(F["T"][reg] - cd[reg]).max() / scale
    print(f"largest |T - central difference| over the region's largest shear rate {scale:.3e}: {dev:.4e}")
    assert scale > 5e-3   # a shear profile is there
    # measured 2.19e-3 of the region's largest shear rate (the same at 3000, 6000 and 12000 steps: the steady state; 5.3e-3 at
    # s8 = s9 = 1.6): the truncation error of the central difference on this profile. Twice that is allowed.
    assert dev <= 4.4e-3
