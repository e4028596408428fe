"""CPU: the host side of write_densities (include/lbmdem_hip.h: lbmdem_write_densities_host, lbmdem_format_fixed4) -- the exact
four-decimal formatter the device uses against "%.4f", the reference's loops over the CPU oracle's f and obst against
tests/golden/densities_*.npz, and the error paths that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import densities_util as du

SYMBOLS = ("lbmdem_write_densities", "lbmdem_download_densities_text", "lbmdem_set_densities_staging", "lbmdem_densities_stats",
           "lbmdem_write_densities_host", "lbmdem_format_fixed4")


def test_symbols_in_header_and_library(pkg):
    declared = pkg.exported_symbols()
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s


def fixed4_values():
    rng = np.random.default_rng(20260418)
    v = [k / 32 for k in range(-200, 201)]
    for k in range(3000):
        t = (k + 0.5) / 1e4
        v += [t, np.nextafter(t, 0.0), np.nextafter(t, 1.0), -t, -np.nextafter(t, 0.0), -np.nextafter(t, 1.0)]
    v += [0.0, -0.0, -4e-5, 5e-5, -5e-5, 9.99995, 0.99995, 99999.99995, 999999999.99994]
    r = 10.0 ** rng.uniform(-6, 5, 100000) * rng.choice([-1.0, 1.0], 100000)
    return np.array(v + r.tolist())


def test_format_fixed4_is_printf(pkg):
    v = fixed4_values()
    got = pkg.format_fixed4(v).split(b"\n")
    assert got[-1] == b"" and len(got) == len(v) + 1
    want = [("%.4f" % float(x)).encode() for x in v]
    bad = [(float(x), g, w) for x, g, w in zip(v, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
    assert pkg.format_fixed4([-0.0, -4e-5, 5e-5, 9.99995]) == b"-0.0000\n-0.0000\n0.0001\n10.0000\n"


def test_format_fixed4_refuses(pkg):
    lib = pkg.load_library()
    n = C.c_long(0)
    out = np.zeros(64, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for bad in (np.nan, np.inf, -np.inf, 1e9, -1e12):
        assert lib.lbmdem_format_fixed4(vp(np.array([1.0, bad])), 2, vp(out), 64, C.byref(n)) == -1
    two = np.array([1.5, -2.25])
    assert lib.lbmdem_format_fixed4(vp(two), 2, vp(out), 5, C.byref(n)) == -1 and n.value == 15   # (the length is reported)
    assert lib.lbmdem_format_fixed4(vp(two), 2, vp(out), 15, C.byref(n)) == 0 and bytes(out[:15]) == b"1.5000\n-2.2500\n"
    assert lib.lbmdem_format_fixed4(None, 2, vp(out), 64, C.byref(n)) == -1
    assert lib.lbmdem_format_fixed4(vp(two), 2, None, 64, C.byref(n)) == -1
    assert lib.lbmdem_format_fixed4(vp(two), 2, vp(out), 64, None) == -1


@pytest.mark.parametrize("name", sorted(du.CASES))
def test_host_writer_gives_the_golden(pkg, po, tmp_path, name):
    f, obst = du.oracle_state(po, name)
    pkg.write_densities_host(str(tmp_path), du.NFILE, f, obst)
    files = du.read_files(tmp_path)
    du.is_golden(files, name)
    want = du.mdg.files(f, obst)
    du.same_text(files[0], want[0].encode(), name)
    du.same_text(files[1], want[1].encode(), name)


def test_host_writer_prints_what_the_device_refuses(pkg, tmp_path):
    """nan, inf and ten digits go through printf; t goes into the header; two rows only: no pressure_base lines"""
    f = np.full((3, 2, 9), 1.0 / 9)
    f[1, 0, 6] = np.inf
    f[1, 1] = 0.0
    f[1, 1, 6] = 1e12
    obst = np.full((3, 2), -1, np.int32)
    obst[0, 0] = 0
    pkg.write_densities_host(str(tmp_path), du.NFILE, f, obst, t=0.125)
    vtk, press = du.read_files(tmp_path)
    assert press == b"" and b"Outfile domain LB t: 1.250000e-01\n" in vtk
    body = du.body_of(vtk.replace(b"t: 1.250000e-01", b"t: 0.000000e+00"), 3, 2).split(b"\n")
    assert body[0] == b"0.0000" and body[1] == b"inf" and body[6 + 4] == b"1000000000000.0000 0.0000 0."
    assert body[6 + 1] == b"inf -nan 0." or body[6 + 1] == b"inf nan 0."


def test_error_paths_without_a_device(pkg, tmp_path):
    lib = pkg.load_library()
    f, obst = np.full((4, 5, 9), 1.0 / 9), np.full((4, 5), -1, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    d = os.fsencode(str(tmp_path))
    host = lib.lbmdem_write_densities_host
    assert host(d, 0, 4, 5, 0.0, 1000.0, None, vp(obst)) == -1
    assert host(d, 0, 4, 5, 0.0, 1000.0, vp(f), None) == -1
    assert host(d, 0, 0, 5, 0.0, 1000.0, vp(f), vp(obst)) == -1 and host(d, 0, 4, 0, 0.0, 1000.0, vp(f), vp(obst)) == -1
    assert host(os.fsencode(str(tmp_path / "no" / "such")), 0, 4, 5, 0.0, 1000.0, vp(f), vp(obst)) == -1
    assert b"cannot open" in lib.lbmdem_last_error()
    assert host(d, 0, 4, 5, 0.0, 1000.0, vp(f), vp(obst)) == 0
    with pytest.raises(pkg.LbmDemError):
        pkg.write_densities_host(str(tmp_path), 0, f, obst[:-1])
    n = C.c_size_t(0)
    for rc in (lib.lbmdem_write_densities(None, d, 0), lib.lbmdem_download_densities_text(None, None, 0, C.byref(n)),
               lib.lbmdem_set_densities_staging(None, 0), lib.lbmdem_densities_stats(None, vp(np.zeros(4, np.int64)))):
        assert rc == -1
