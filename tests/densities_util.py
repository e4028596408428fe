"""Shared by the write_densities tests: the generator of tests/golden/densities_*.npz (its case list, its sequence and its
restatement of main.c:482-566), the goldens, the CPU oracle's state per case, and the comparison of two texts."""
import hashlib
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_densities_golden", os.path.join(HERE, "golden", "make_densities_golden.py"))
mdg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mdg)

CASES = mdg.cases()
NFILE = mdg.NFILE
NAMES = ("densities%06d.vtk" % NFILE, "pressure_base%06d.dat" % NFILE)
_golden, _oracle = {}, {}


def golden(name):
    if name not in _golden:
        g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
        for v in g.values():
            v.setflags(write=False)
        _golden[name] = g
    return _golden[name]


def oracle_state(po, name):
    """(f, obst) of the CPU oracle after the case's sequence, computed once"""
    if name not in _oracle:
        case = CASES[name]
        ora = po.Oracle(case["lx"], case["ly"], *mdg.grains_m(case))
        mdg.drive(ora, case, ora.scalars()["npDEM"])
        f, obst = ora.get_f(), ora.get_obst()
        f.setflags(write=False)
        obst.setflags(write=False)
        _oracle[name] = (f, obst)
    return _oracle[name]


def read_files(directory):
    return tuple(open(os.path.join(directory, n), "rb").read() for n in NAMES)


def same_text(got, want, what=""):
    """two texts (bytes), compared whole; the first differing line is reported"""
    if got == want:
        return
    a, b = got.split(b"\n"), want.split(b"\n")
    for k, (x, y) in enumerate(zip(a, b)):
        assert x == y, (what, "line", k, x[:80], y[:80])
    assert len(a) == len(b), (what, "lines", len(a), len(b))


def body_of(vtk, lx, ly):
    """the file without its header lines and without the line between the sections: what densities_text() returns"""
    head = mdg.header(lx, ly).encode()
    assert vtk.startswith(head)
    rest = vtk[len(head):]
    k = rest.index(mdg.VELOCITY_HEAD.encode())
    return rest[:k] + rest[k + len(mdg.VELOCITY_HEAD):]


def first_bad_row(vtk, g, lx, ly):
    """the first file row (section, y) whose byte count is not the golden's, or None"""
    lines = body_of(vtk, lx, ly).split(b"\n")[:-1]
    for s in range(2):
        for y in range(ly):
            n = sum(len(l) + 1 for l in lines[(s * ly + y) * lx:(s * ly + y + 1) * lx])
            if n != int(g["row_bytes"][s, y]):
                return ("pressure", "velocity")[s], y, n, int(g["row_bytes"][s, y])
    return None


def is_golden(files, name):
    """the two files have the golden's sha256 and byte counts; on a mismatch the first differing file row is named"""
    g, case = golden(name), CASES[name]
    vtk, press = files
    if hashlib.sha256(vtk).hexdigest() != str(g["vtk_sha256"]):
        bad = first_bad_row(vtk, g, case["lx"], case["ly"])
        rows = body_of(vtk, case["lx"], case["ly"])
        at = 0
        for s, key in enumerate(("p_row_%d", "v_row_%d")):   # (equal byte counts: compare the rows the golden keeps)
            for y in range(case["ly"]):
                n = int(g["row_bytes"][s, y])
                if bad is None and key % y in g and rows[at:at + n] != bytes(g[key % y]):
                    bad = (key % y, "text differs")
                at += n
        raise AssertionError((name, "densities file differs from the golden", len(vtk), int(g["vtk_bytes"]), bad))
    assert len(vtk) == int(g["vtk_bytes"])
    assert press == bytes(g["press_text"]) and hashlib.sha256(press).hexdigest() == str(g["press_sha256"])
    assert len(press) == int(g["press_bytes"])
