"""CPU: the host side of the tables written in the background -- lbmdem_write_dem_rows, the formatter and the pair search that
lbmdem_write_dem / lbmdem_write_forces and the writer thread share, against the files the reference wrote
(tests/golden/dem_G6_4000steps/): rows built from the reference's own 30-column table give DEM000000.dat character for
character, the stats.data line field for field and DEM000000.ps under the header rule of tests/test_gpu_dem_output.py; and
the new entry points are declared and exported."""
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu

REF_DIR = os.path.join(gu.HERE, "golden", "dem_G6_4000steps")
DEM_SYMBOLS = ("lbmdem_dem_stats", "lbmdem_set_async_dem", "lbmdem_write_dem_async", "lbmdem_output_stats_dem",
               "lbmdem_write_dem_rows")
LX, LY = 256, 200


def golden_rows(po):
    """(n, 28) rows in the file's order from the reference's table; fhf1..3 and ESE, which the table does not hold, parsed
    from the reference's DEM000000.dat (a %le value parsed and printed again gives the same text)"""
    t = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))["grains"]
    dat = np.array([[float(v) for v in l.split("\t")] for l in open(os.path.join(REF_DIR, "DEM000000.dat")).read().splitlines()])
    assert dat.shape == (len(t), 28)
    c = po.COL
    rows = np.zeros((len(t), 28))
    rows[:, 0] = t[:, c["r"]]
    for k, name in enumerate("x1 x2 x3 v1 v2 v3 a1 a2 a3".split()):
        rows[:, 1 + k] = t[:, c[name]]
    rows[:, 10:13] = dat[:, 11:14]                  # fhf1..3 (column 0 of the file is the index)
    rows[:, 13], rows[:, 14] = t[:, c["p"]], t[:, c["s"]]
    rows[:, 15] = dat[:, 16]                        # ESE
    for k, name in enumerate("fr ifr ice slip rw fm M11 M12 M21 M22 z zz".split()):
        rows[:, 16 + k] = t[:, c[name]]
    return rows


def golden_stats():
    return np.array([float(v) for v in open(os.path.join(REF_DIR, "stats.data")).read().split()])


def check_against_golden(d):
    """the rules of tests/test_gpu_dem_output.py::test_dem_file_and_stats_line_match_the_reference"""
    assert (d / "DEM000000.dat").read_text() == open(os.path.join(REF_DIR, "DEM000000.dat")).read()
    got = (d / "DEM000000.ps").read_bytes().split(b"\n")
    want = open(os.path.join(REF_DIR, "DEM000000.ps"), "rb").read().split(b"\n")
    assert got[1].startswith(b"%%BoundingBox: ") and got[2].startswith(b"%%Creator") and got[3].startswith(b"%%Title")
    assert [got[0]] + got[4:] == want      # the fixture has the three undefined header lines removed
    assert sum(l.startswith(b"stroke") for l in got) >= 20


def test_rows_reproduce_the_reference_files(pkg, po, tmp_path):
    rows, st = golden_rows(po), golden_stats()
    assert st.shape == (22,)
    pkg.write_dem_rows(str(tmp_path), 0, rows, st, forces=True, lx=LX, ly=LY)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["DEM000000.dat", "DEM000000.ps", "stats.data"]
    check_against_golden(tmp_path)
    sw = open(os.path.join(REF_DIR, "stats.data")).read().split()
    lines = (tmp_path / "stats.data").read_text().splitlines()
    assert len(lines) == 1 and lines[0].split() == sw and len(sw) == 22
    # the bounding box is the lattice's, with a margin of ten radii of grain 0
    m = 10 * rows[0, 0]
    assert (tmp_path / "DEM000000.ps").read_bytes().split(b"\n")[1] == \
        ("%%%%BoundingBox: %f %f %f %f " % (-m, -m, LX + m, LY + m)).encode()
    # a second event appends a second line and, without the map, leaves the first one's alone
    ps = (tmp_path / "DEM000000.ps").read_bytes()
    st2 = st.copy(); st2[0] += 1.0
    pkg.write_dem_rows(str(tmp_path), 1, rows, st2, forces=False, lx=LX, ly=LY)
    lines = (tmp_path / "stats.data").read_text().splitlines()
    assert len(lines) == 2 and lines[0].split() == sw and lines[1].split()[1:] == sw[1:] and lines[1].split()[0] == "%le" % st2[0]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["DEM000000.dat", "DEM000000.ps", "DEM000001.dat", "stats.data"]
    assert (tmp_path / "DEM000001.dat").read_bytes() == (tmp_path / "DEM000000.dat").read_bytes()
    assert (tmp_path / "DEM000000.ps").read_bytes() == ps


def test_one_grain_and_a_table_without_contacts(pkg, tmp_path):
    """n = 1: no pair to search, a grid of one cell"""
    rows = np.zeros((1, 28))
    rows[0, :3] = (0.7e-3, 3e-3, 2e-3)
    pkg.write_dem_rows(str(tmp_path), 7, rows, np.arange(22.0), forces=True, lx=64, ly=48)
    dat = (tmp_path / "DEM000007.dat").read_text().splitlines()
    assert len(dat) == 1 and dat[0].split("\t")[:4] == ["0", "%le" % 0.7e-3, "%le" % 3e-3, "%le" % 2e-3] and dat[0].endswith("\t0")
    ps = (tmp_path / "DEM000007.ps").read_text().splitlines()
    assert len(ps) == 6 and ps[5].startswith("newpath ") and not any(l.startswith("stroke") for l in ps)
    assert (tmp_path / "stats.data").read_text().split() == ["%le" % v for v in range(22)]


def test_refusals(pkg, po, tmp_path):
    rows, st = golden_rows(po), golden_stats()
    missing = str(tmp_path / "no" / "such" / "dir")
    with pytest.raises(pkg.LbmDemError) as e:
        pkg.write_dem_rows(missing, 0, rows, st)
    assert e.value.code == -1 and missing in str(e.value)
    L = pkg.load_library()
    d = os.fsencode(str(tmp_path))
    vp = lambda a: a.ctypes.data
    assert L.lbmdem_write_dem_rows(d, 0, 0, vp(rows), vp(st), 1, LX, LY) == -1
    assert b"lbmdem_write_dem_rows" in L.lbmdem_last_error()
    assert L.lbmdem_write_dem_rows(d, 0, len(rows), None, vp(st), 1, LX, LY) == -1
    assert L.lbmdem_write_dem_rows(d, 0, len(rows), vp(rows), None, 1, LX, LY) == -1
    with pytest.raises(pkg.LbmDemError):     # rows of the wrong width never reach the library
        pkg.write_dem_rows(str(tmp_path), 0, rows[:, :27], st)
    assert [p.name for p in tmp_path.iterdir()] == []


def test_header_declares_and_libraries_export_the_entry_points(pkg):
    names = pkg.exported_symbols()
    assert set(DEM_SYMBOLS) <= set(names)
    header = open(pkg.HEADER_PATH).read()
    assert "#define LBMDEM_DEM_ROW_DOUBLES 28" in header and "#define LBMDEM_ASYNC_MAX_DEM 4" in header
    assert pkg.DEM_ROW_DOUBLES == 28
    L = pkg.load_library()
    assert all(hasattr(L, n) for n in DEM_SYMBOLS)
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):     # same ABI: the float library has the symbols and refuses the device ones
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(DEM_SYMBOLS) <= exported, (path, sorted(set(DEM_SYMBOLS) - exported))
        assert all(n.startswith("lbmdem_") for n in exported), sorted(n for n in exported if not n.startswith("lbmdem_"))[:5]


def test_null_handle_is_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    assert L.lbmdem_dem_stats(None, None) == -1
    assert L.lbmdem_set_async_dem(None, 2) == -1
    assert L.lbmdem_write_dem_async(None, b".", 0, 1, None) == -1
    assert L.lbmdem_output_stats_dem(None, None, None) == -1
    assert b"null handle" in L.lbmdem_last_error()


def test_host_driver_documents_and_refuses_the_flag_with_several_gpus(tmp_path):
    root = os.path.dirname(gu.HERE)
    exe = os.path.join(root, "2d-lbm-dem_amd", "host", "lbmdem")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    out = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert "--async-dem [N]" in out.stdout
    for extra in (["--gpus", "2"], ["--comm"], ["3", "--gpus", "2"]):
        args = [exe, "nothing.data", "--async-dem"] + extra
        out = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert out.returncode != 0 and "--async-dem is a single-GPU mode" in out.stderr, (args, out.stderr)
