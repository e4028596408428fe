"""CPU: lbmdem_write_contacts_files (include/lbmdem_hip.h), the host-only formatter of the contact network export --
contacts%.6i.dat and DEM%.6i_chains.ps from hand-made records -- and the record's layout. No device is touched."""
import ctypes

import numpy as np
import pytest

import contacts_util as cu


def _grains():
    r = np.array([0.5e-3, 0.75e-3, 0.6e-3])
    x1 = np.array([1.0e-3, 2.2e-3, 3.5e-3])
    x2 = np.array([0.5e-3, 0.7e-3, 0.6e-3])
    fm = np.array([0.0, 0.25, 1.0])
    return r, x1, x2, fm


def _records():
    rec = np.zeros(4, cu.CONTACT_DTYPE)
    rec[0] = (0, 1, -1.5e-6, -0.986, -0.164, 2.4, -0.3)
    rec[1] = (1, 2, -1e-7, -1.0, 0.0, 0.0, 0.0)                 # touching, fn clamped to 0
    rec[2] = (0, cu.WALL_B, -2e-6, 0.0, 1.0, 6.0, 1.25e-300)    # walls follow the pairs
    rec[3] = (2, cu.WALL_R, -3e-6, -1.0, 0.0, -9.0, 4.194e+250)
    return rec


def _expected(nfile, r, x1, x2, fm, rec, lx, ly):
    dat = "# i j dn nx ny fn ft\n" + "".join(
        "%d %d %e %e %e %e %e\n" % (c["i"], c["j"], c["dn"], c["nx"], c["ny"], c["fn"], c["ft"]) for c in rec)
    m = 10 * r[0]
    ps = "%!PS-Adobe-3.0 EPSF-3.0 \n"
    ps += "%%%%BoundingBox: %f %f %f %f \n" % (-m, -m, lx + m, ly + m)
    ps += "%%Creator: lbmdem-hip \n%%Title: DEM Grains & Forces \n0.1 setlinewidth 0.0 setgray \n"
    for i in range(len(r)):
        ps += "newpath %e %e %e 0.0 setlinewidth %.2f setgray 0 360 arc gsave fill grestore\n" % (
            x1[i] * 10000, x2[i] * 10000, r[i] * 10000, 0.8 - fm[i] / 2)
    for c in rec:
        if c["j"] >= 0 and c["fn"] > 0:
            i, j = c["i"], c["j"]
            ps += "%e setlinewidth \n 0.0 setgray \n" % c["fn"]
            ps += "1 setlinecap \n newpath \n"
            ps += "%e %e moveto \n %e %e lineto\n" % (x1[i] * 10000, x2[i] * 10000, x1[j] * 10000, x2[j] * 10000)
            ps += "stroke \n"
    return dat, ps


def test_record_is_48_bytes(pkg):
    assert ctypes.sizeof(pkg.Contact) == 48
    assert pkg.CONTACT_DTYPE.itemsize == 48 and cu.CONTACT_DTYPE == pkg.CONTACT_DTYPE
    assert [f[0] for f in pkg.Contact._fields_] == list(pkg.CONTACT_DTYPE.names)
    assert [getattr(pkg.Contact, n).offset for n in pkg.CONTACT_DTYPE.names] == [pkg.CONTACT_DTYPE.fields[n][1] for n in pkg.CONTACT_DTYPE.names]
    assert (pkg.WALL_B, pkg.WALL_T, pkg.WALL_L, pkg.WALL_R) == (-1, -2, -3, -4) == (cu.WALL_B, cu.WALL_T, cu.WALL_L, cu.WALL_R)


def test_files_are_exactly_the_expected_text(pkg, tmp_path):
    r, x1, x2, fm = _grains()
    rec = _records()
    pkg.write_contacts_files(str(tmp_path), 7, r, x1, x2, fm, rec, 64, 48)
    dat, ps = _expected(7, r, x1, x2, fm, rec, 64, 48)
    got_dat = (tmp_path / "contacts000007.dat").read_text()
    got_ps = (tmp_path / "DEM000007_chains.ps").read_text()
    assert got_dat == dat
    assert got_ps == ps
    # the fn == 0 pair is a record of the table and no chain of the map; walls never reach the map
    assert len(got_dat.splitlines()) == 1 + len(rec) and "1 2 " in got_dat
    assert got_ps.count("stroke") == 1
    assert "%e setlinewidth" % 6.0 not in got_ps and "%e setlinewidth" % -9.0 not in got_ps


def test_empty_list_writes_header_and_discs_only(pkg, tmp_path):
    r, x1, x2, fm = _grains()
    pkg.write_contacts_files(str(tmp_path), 0, r, x1, x2, fm, np.zeros(0, cu.CONTACT_DTYPE), 64, 48)
    assert (tmp_path / "contacts000000.dat").read_text() == "# i j dn nx ny fn ft\n"
    ps = (tmp_path / "DEM000000_chains.ps").read_text()
    assert ps.count("newpath") == 3 and "stroke" not in ps


def test_missing_directory_is_refused(pkg, tmp_path):
    r, x1, x2, fm = _grains()
    with pytest.raises(pkg.LbmDemError, match="cannot open"):
        pkg.write_contacts_files(str(tmp_path / "not" / "there"), 0, r, x1, x2, fm, _records(), 64, 48)


def test_null_and_bad_arguments_are_refused(pkg, tmp_path):
    L = pkg.load_library()
    r, x1, x2, fm = _grains()
    rec = _records()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    d = str(tmp_path).encode()
    ok = [d, 0, 3, vp(r), vp(x1), vp(x2), vp(fm), vp(rec), len(rec), 64, 48]
    for k in (3, 4, 5, 6, 7):
        args = list(ok)
        args[k] = None
        assert L.lbmdem_write_contacts_files(*args) == -1, k      # LBMDEM_EINVAL
    args = list(ok); args[2] = 0
    assert L.lbmdem_write_contacts_files(*args) == -1
    args = list(ok); args[8] = -1
    assert L.lbmdem_write_contacts_files(*args) == -1
    bad = rec.copy(); bad["j"][0] = 3                              # a grain that does not exist
    args = list(ok); args[7] = vp(bad)
    assert L.lbmdem_write_contacts_files(*args) == -1
    bad = rec.copy(); bad["j"][2] = -5                             # no such wall
    args = list(ok); args[7] = vp(bad)
    assert L.lbmdem_write_contacts_files(*args) == -1
    assert L.lbmdem_write_contacts_files(*ok) == 0


def test_both_libraries_export_the_formatter(pkg, tmp_path):
    import os
    if not os.path.exists(pkg.SP_LIB_PATH):
        pytest.skip("the single-precision library has not been built")
    r, x1, x2, fm = _grains()
    rec = _records()
    pkg.write_contacts_files(str(tmp_path), 1, r, x1, x2, fm, rec, 64, 48, precision="f32")
    dat, ps = _expected(1, r, x1, x2, fm, rec, 64, 48)
    assert (tmp_path / "contacts000001.dat").read_text() == dat
    assert (tmp_path / "DEM000001_chains.ps").read_text() == ps
