"""CPU: the host-only half of the coarse-grained fields (include/lbmdem_hip.h) -- lbmdem_coarse_grid's arithmetic and
lbmdem_write_coarse_files, the formatter of coarse%.6i.dat, from a hand-made grid -- and the record's layout. No device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import coarse_util as cz

SYMBOLS = ("lbmdem_coarse_grid", "lbmdem_coarse_fields", "lbmdem_write_coarse", "lbmdem_write_coarse_files",
           "lbmdem_set_coarse_output")


def _cells():
    """a 3 x 2 grid (lx = 5, ly = 3 with cells of 2 x 2), every member different, with a negative value and a zero"""
    cells = np.zeros((3, 2), cz.DTYPE)
    for k, name in enumerate(cz.FIELDS):
        cells[name] = (np.arange(6).reshape(3, 2) + 1) * (k + 1) * 1.25e-3
    cells["sum_jx"][1, 0] = -4.5e-7
    cells["sum_mv2"][2, 1] = -1.0e+200
    cells["grains"][0, 1] = 0.0
    cells["M12"][2, 0] = 0.0
    return cells


def test_record_is_25_doubles(pkg):
    assert pkg.COARSE_DTYPE == cz.DTYPE and pkg.COARSE_DTYPE.itemsize == 25 * 8
    assert list(pkg.COARSE_DTYPE.names) == cz.FIELDS
    header = open(pkg.HEADER_PATH).read()
    assert "#define LBMDEM_COARSE_DOUBLES 25" in header
    body = header.split("typedef struct lbmdem_coarse_cell {")[1].split("}")[0]
    assert [w.strip(" ;\n") for w in body.replace("double", "").replace(";", ",").split(",") if w.strip(" ;\n")] == cz.FIELDS


@pytest.mark.parametrize("lx,ly,cw,ch,want", [
    (256, 200, 16, 16, (16, 13)), (256, 200, 7, 13, (37, 16)), (256, 200, 1, 1, (256, 200)), (256, 200, 256, 200, (1, 1)),
    (256, 200, 300, 300, (1, 1)), (256, 200, 257, 199, (1, 2)), (61, 59, 60, 60, (2, 1)), (1, 1, 1, 1, (1, 1)),
    (4096, 4096, 64, 64, (64, 64)), (5, 3, 2 ** 31 - 1, 2 ** 31 - 1, (1, 1))])
def test_grid_arithmetic(pkg, lx, ly, cw, ch, want):
    assert pkg.coarse_grid(lx, ly, cw, ch) == want == cz.grid(lx, ly, cw, ch)


def test_grid_refuses_cells_without_nodes(pkg):
    for cw, ch in ((0, 16), (16, 0), (0, 0), (-1, 4)):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.coarse_grid(256, 200, cw, ch)
        assert e.value.code == -1
    L = pkg.load_library()
    n = ctypes.c_int(0)
    assert L.lbmdem_coarse_grid(256, 200, 16, 16, None, ctypes.byref(n)) == -1
    assert L.lbmdem_coarse_grid(256, 200, 16, 16, ctypes.byref(n), None) == -1
    assert L.lbmdem_coarse_grid(0, 200, 16, 16, ctypes.byref(n), ctypes.byref(n)) == -1


def test_file_is_exactly_the_expected_text(pkg, tmp_path):
    cells = _cells()
    pkg.write_coarse_files(str(tmp_path), 7, 5, 3, 2, 2, cells, outside=3, contacts_valid=1)
    got = (tmp_path / "coarse000007.dat").read_text()
    want = "# cw %d ch %d ncx %d ncy %d outside %d contacts %d\n" % (2, 2, 3, 2, 3, 1)
    for cx in range(3):
        for cy in range(2):
            want += "%d %d" % (cx, cy) + "".join(" %e" % cells[name][cx, cy] for name in cz.FIELDS) + "\n"
    assert got == want == cz.file_text(2, 2, cells, 3, 1)
    lines = got.splitlines()
    assert len(lines) == 7 and all(len(l.split()) == 27 for l in lines[1:])
    assert [l.split()[:2] for l in lines[1:]] == [["0", "0"], ["0", "1"], ["1", "0"], ["1", "1"], ["2", "0"], ["2", "1"]]
    assert " -4.500000e-07 " in lines[3] and " -1.000000e+200 " in lines[6] and " 0.000000e+00 " in lines[2]
    assert sorted(os.listdir(tmp_path)) == ["coarse000007.dat"]


def test_missing_directory_is_refused(pkg, tmp_path):
    with pytest.raises(pkg.LbmDemError, match="cannot open") as e:
        pkg.write_coarse_files(str(tmp_path / "not" / "there"), 0, 5, 3, 2, 2, _cells())
    assert e.value.code == -1


def test_null_and_bad_arguments_are_refused(pkg, tmp_path):
    L = pkg.load_library()
    cells = _cells()
    d = str(tmp_path).encode()
    p = cells.ctypes.data_as(ctypes.c_void_p)
    assert L.lbmdem_write_coarse_files(d, 0, 5, 3, 2, 2, None, 0, 0) == -1
    assert L.lbmdem_write_coarse_files(d, 0, 5, 3, 0, 2, p, 0, 0) == -1
    assert L.lbmdem_write_coarse_files(d, 0, 5, 3, 2, -2, p, 0, 0) == -1
    assert os.listdir(tmp_path) == []
    assert L.lbmdem_write_coarse_files(d, 0, 5, 3, 2, 2, p, 0, 0) == 0
    with pytest.raises(pkg.LbmDemError, match="shape"):
        pkg.write_coarse_files(str(tmp_path), 0, 5, 3, 2, 2, cells[:2])
    # no handle: refused before any device is looked for
    assert L.lbmdem_coarse_fields(None, 2, 2, None, 0, None, None) == -1
    assert L.lbmdem_write_coarse(None, d, 0, 2, 2) == -1
    assert L.lbmdem_set_coarse_output(None, 2, 2) == -1


def test_host_driver_refuses_bad_coarse_arguments(pkg):
    """`lbmdem --coarse CWxCH` is refused with --gpus N, like --contacts, and for anything that is not two counts; all of it
    before a file is read or a device looked for"""
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "host", "lbmdem")
    run = lambda *a: subprocess.run([exe, "no_such_sample.data", *a], capture_output=True, text=True)
    out = run("--coarse", "16x16", "--gpus", "2")
    assert out.returncode != 0 and "--coarse is a single-GPU mode" in out.stderr
    for bad in ("16", "0x4", "4x0", "4x4z", "x"):
        out = run("--coarse", bad)
        assert out.returncode != 0 and "--coarse CWxCH" in out.stderr, bad
    out = run("--coarse")
    assert out.returncode != 0 and "--coarse CWxCH" in out.stderr


def test_both_libraries_export_the_symbols(pkg, tmp_path):
    assert set(SYMBOLS) <= set(pkg.exported_symbols())
    assert os.path.exists(pkg.SP_LIB_PATH), "the single-precision library has not been built"
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(SYMBOLS) <= exported, path
    # the two host-only calls work in the float library too
    assert pkg.coarse_grid(256, 200, 7, 13, precision="f32") == (37, 16)
    cells = _cells()
    pkg.write_coarse_files(str(tmp_path), 1, 5, 3, 2, 2, cells, outside=2, contacts_valid=0, precision="f32")
    assert (tmp_path / "coarse000001.dat").read_text() == cz.file_text(2, 2, cells, 2, 0)
