"""CPU: the probe recorder's declarations are in include/lbmdem_hip.h and exported by both libraries (same ABI); the
Python structure matches the C one field for field."""
import ctypes as C
import re
import subprocess

PROBE_SYMBOLS = ("lbmdem_probe_enable", "lbmdem_probe_disable", "lbmdem_probe_record_doubles", "lbmdem_probe_layout",
                 "lbmdem_probe_read")


def test_header_declares_the_probe_entry_points(pkg):
    names = pkg.exported_symbols()
    assert set(PROBE_SYMBOLS) <= set(names)
    txt = open(pkg.HEADER_PATH).read()
    m = re.search(r"typedef struct lbmdem_probe_config \{(.*?)\} lbmdem_probe_config;", txt, re.S)
    assert m, "lbmdem_probe_config is not declared"
    fields = re.findall(r"\b(?:const\s+)?int\s*\*?\s*(\w+)\s*;", m.group(1))
    assert fields == ["every", "capacity", "pressure_row", "velocity_row", "npoints", "points", "grain_extent"]
    assert [f[0] for f in pkg.ProbeConfig._fields_] == fields
    assert "#define LBMDEM_PROBE_MAX_POINTS 64" in txt


def test_libraries_export_the_probe_entry_points(pkg):
    for path in (pkg.LIB_PATH, pkg.SP_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert set(PROBE_SYMBOLS) <= exported, (path, sorted(set(PROBE_SYMBOLS) - exported))
        assert all(n.startswith("lbmdem_") for n in exported)


def test_null_handle_is_refused_without_a_gpu(pkg):
    L = pkg.load_library()
    assert L.lbmdem_probe_disable(None) == -1
    assert L.lbmdem_probe_enable(None, C.byref(pkg.ProbeConfig())) == -1
    assert L.lbmdem_probe_record_doubles(None) == -1
    assert L.lbmdem_probe_read(None, None, 0, None, None) == -1
    assert b"null handle" in L.lbmdem_last_error()
