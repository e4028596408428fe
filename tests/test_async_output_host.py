"""CPU: the background frame writer's host side -- its entry points are declared and exported (both libraries, same ABI),
the size of a frame image, and the host-only image writer against the reference's own VTK files: their payloads cut off,
glued into an image and written again give the same five files byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as gu

ASYNC_SYMBOLS = ("lbmdem_set_async_output", "lbmdem_write_vtk_async", "lbmdem_output_drain", "lbmdem_output_stats",
                 "lbmdem_vtk_image_bytes", "lbmdem_write_vtk_image", "lbmdem_download_vtk_image")
# the image's order, with the floats per node
FIELDS = (("grain_pressure", 1), ("grain_velocity", 3), ("grain_acceleration", 3), ("fluid_pressure", 1), ("fluid_velocity", 3))
GOLDEN = os.path.join(gu.HERE, "golden", "vtk_G5_25steps")
LX, LY, NFILE = 64, 48, 3


def golden_image():
    parts = []
    for name, dim in FIELDS:
        blob = open(os.path.join(GOLDEN, "%s_%06d.vtk" % (name, NFILE)), "rb").read()
        parts.append(blob[len(blob) - LX * LY * 4 * dim:])
    return b"".join(parts)


def test_header_declares_and_libraries_export_the_entry_points(pkg):
    names = pkg.exported_symbols()
    assert set(ASYNC_SYMBOLS) <= set(names)
    assert "#define LBMDEM_ASYNC_MAX_FRAMES 4" in open(pkg.HEADER_PATH).read()
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(ASYNC_SYMBOLS) <= exported, (path, sorted(set(ASYNC_SYMBOLS) - exported))
        assert all(n.startswith("lbmdem_") for n in exported), sorted(n for n in exported if not n.startswith("lbmdem_"))[:5]
        if path == pkg.LIB_PATH:
            assert set(names) <= exported


def test_image_size(pkg):
    assert pkg.vtk_image_bytes(64, 48) == 44 * 64 * 48
    assert pkg.vtk_image_bytes(4096, 4096) == 44 * 4096 * 4096      # beyond 2^29: no 32-bit product on the way
    assert pkg.vtk_image_bytes(0, 48) == 0


def test_image_writer_reproduces_the_reference_files(pkg, tmp_path):
    image = golden_image()
    assert len(image) == pkg.vtk_image_bytes(LX, LY)
    pkg.write_vtk_image(str(tmp_path), NFILE, LX, LY, image)
    names = sorted(os.listdir(GOLDEN))
    assert len(names) == 5 and sorted(p.name for p in tmp_path.iterdir()) == names
    for name in names:
        got, want = (tmp_path / name).read_bytes(), open(os.path.join(GOLDEN, name), "rb").read()
        assert got == want, f"{name}: {len(got)} vs {len(want)} bytes, first diff at " \
                            f"{next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)}"
    # a numpy array of the same bytes is taken as well
    other = tmp_path / "again"
    other.mkdir()
    pkg.write_vtk_image(str(other), NFILE, LX, LY, np.frombuffer(image, np.uint8))
    for name in names:
        assert (other / name).read_bytes() == (tmp_path / name).read_bytes()


def test_image_writer_agrees_with_the_field_writer(pkg, tmp_path):
    """lbmdem_write_vtk_fields (host floats, swapped on the host) and lbmdem_write_vtk_image (bytes as they stand) on the same
    values, on a lattice that is not the golden one"""
    lx, ly = 37, 21
    rng = np.random.default_rng(3)
    fields = rng.normal(size=11 * lx * ly).astype(np.float32)
    a, b = tmp_path / "fields", tmp_path / "image"
    a.mkdir(); b.mkdir()
    pkg.write_vtk_fields(str(a), 12, lx, ly, fields)
    pkg.write_vtk_image(str(b), 12, lx, ly, fields.astype(">f4").tobytes())
    names = sorted(p.name for p in a.iterdir())
    assert len(names) == 5 and names == sorted(p.name for p in b.iterdir())
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n


def test_image_writer_refusals(pkg, tmp_path):
    image = golden_image()
    missing = str(tmp_path / "no" / "such" / "dir")
    with pytest.raises(pkg.LbmDemError) as e:
        pkg.write_vtk_image(missing, NFILE, LX, LY, image)
    assert e.value.code == -1 and missing in str(e.value)
    L = pkg.load_library()
    buf = C.create_string_buffer(image)
    for lx, ly in ((1, 48), (64, 1), (0, 0), (-3, 48)):
        assert L.lbmdem_write_vtk_image(os.fsencode(str(tmp_path)), 0, lx, ly, buf) == -1
        assert b"lbmdem_write_vtk_image" in L.lbmdem_last_error()
    assert L.lbmdem_write_vtk_image(os.fsencode(str(tmp_path)), 0, LX, LY, None) == -1
    with pytest.raises(pkg.LbmDemError):     # an image of the wrong size never reaches the library
        pkg.write_vtk_image(str(tmp_path), 0, LX, LY, image[:-4])
    assert list(tmp_path.iterdir()) == []


def test_null_handle_is_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    assert L.lbmdem_set_async_output(None, 2) == -1
    assert L.lbmdem_write_vtk_async(None, b".", 0) == -1
    assert L.lbmdem_output_drain(None) == -1
    assert L.lbmdem_output_stats(None, None, None) == -1
    assert L.lbmdem_download_vtk_image(None, None) == -1
    assert b"null handle" in L.lbmdem_last_error()


def test_nothing_new_computes_on_the_cpu(pkg):
    """the image comes from the device only: without one there is no handle to ask (as test_abi.py::test_no_cpu_fallback)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LbmDemError) as e:
        pkg.LbmDem(64, 48, [0.7e-3], [3e-3], [3e-3])
    assert e.value.code in (-2, -3)


def test_host_driver_documents_and_refuses_the_flag_with_several_gpus(tmp_path):
    root = os.path.dirname(gu.HERE)
    exe = os.path.join(root, "2d-lbm-dem_amd", "host", "lbmdem")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    out = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert "--async-output [N]" in out.stdout
    for extra in (["--gpus", "2"], ["--comm"], ["3", "--gpus", "2"]):
        args = [exe, "nothing.data", "--async-output"] + extra
        out = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=60)
        assert out.returncode != 0 and "--async-output is a single-GPU mode" in out.stderr, (args, out.stderr)
