"""Shared by the boundary-link tests: the generator of tests/golden/links_*.npz (its case list, its sequence and its
restatement of the link definition), the goldens, and the text of obst_writing's three files (main.c:1601-1641)."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_links_golden", os.path.join(HERE, "golden", "make_links_golden.py"))
mlg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mlg)

CASES = mlg.cases()
CLEAN = sorted(k for k in CASES if CASES[k]["clean"])
FILES = ("obst_LB.dat", "active_nodes.dat", "links.dat")
_cache = {}


def golden(name):
    """the golden's arrays + `delta` [lx][ly][9], `links` (its effective links, file order) and `census` (the six counters)"""
    if name not in _cache:
        g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
        n = len(g["r_mm"])
        g["act"] = g["act"].astype(np.int32)
        g["delta"] = np.zeros(g["obst"].shape + (9,))
        g["delta"][g["delta_x"], g["delta_y"], g["delta_q"]] = g["delta_v"]
        g["links"] = mlg.effective_links(g["obst"], g["act"], g["delta"], n)
        g["census"] = mlg.census(g["obst"], g["act"], g["links"], n)
        for v in g.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def same_links(got, want, what=""):
    """two link lists, bit for bit (delta as its 64 bits)"""
    assert len(got) == len(want), (what, len(got), len(want))
    for k in ("x", "y", "q", "grain"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["delta"].view(np.uint64), want["delta"].view(np.uint64)), (what, "delta")


def map_text(a):
    """main.c:1606-1612: "%d " per node, "\\n" per y"""
    return "".join("".join("%d " % v for v in a[:, y]) + "\n" for y in range(a.shape[1]))


def links_text(x, y, q, d):
    """main.c:1631-1639: one line per entry, delta != 0"""
    return "".join("%d  %d  %d  %f\n" % (a, b, c, v) for a, b, c, v in zip(x.tolist(), y.tolist(), q.tolist(), d.tolist()) if v != 0)


def read_files(directory):
    return tuple(open(os.path.join(directory, f)).read() for f in FILES)
