"""GPU: write_densities with its text made on the device -- the two files against the text restated from the oracle's f and
obst and against tests/golden/densities_*.npz (the unmodified reference), whatever the staging budget cuts the file rows
into; every width of a line and the ties of the rounding on a crafted lattice; the host path for what the device does not
format; that it changes nothing a later step reads; `lbmdem --densities`; the refusals."""
import os
import subprocess

import numpy as np
import pytest

import densities_util as du

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
RAGGED = "densities_a08d83_98x119"


def make(pkg, case, **kw):
    return pkg.LbmDem(case["lx"], case["ly"], *du.mdg.grains_m(case), **kw)


def driven(pkg, name):
    case = du.CASES[name]
    sim = make(pkg, case)
    du.mdg.drive(sim, case, sim.cfg.npDEM, step="renderScene")
    return sim


def written(sim, tmp_path, sub):
    d = tmp_path / sub
    d.mkdir()
    sim.write_densities(str(d), du.NFILE)
    return du.read_files(d)


@pytest.mark.parametrize("name", sorted(du.CASES))
def test_files_are_the_references(pkg, po, tmp_path, name):
    case = du.CASES[name]
    sim = driven(pkg, name)
    files = written(sim, tmp_path, "a")
    f, obst = du.oracle_state(po, name)
    want = du.mdg.files(f, obst)
    du.same_text(files[0], want[0].encode(), name)
    du.same_text(files[1], want[1].encode(), name)
    du.is_golden(files, name)
    g = du.golden(name)
    st = sim.densities_stats()
    assert st[:2] == (int(g["row_bytes"][0].sum()), int(g["row_bytes"][1].sum())) and st[2] == 2 and st[3] == 0
    text = sim.densities_text()
    du.same_text(text, du.body_of(files[0], case["lx"], case["ly"]), name + " densities_text")
    assert sim.densities_stats() == st


def test_band_edges(pkg, tmp_path):
    """98 x 119, budgets of one, 16 and 17 file rows' worth (of the file's longest row): the same bytes as with the default
    budget. densities_stats()[2] counts the bands of BOTH sections together: a section's bands hold as many rows as the budget
    has room for that section's longest row, so the velocity section takes ceil(119 / k) bands and the pressure section, whose
    rows are shorter, ceil(119 / k') with k' = budget // its longest row."""
    case, g = du.CASES[RAGGED], du.golden(RAGGED)
    ly = case["ly"]
    sim = driven(pkg, RAGGED)
    base = written(sim, tmp_path, "default")
    du.is_golden(base, RAGGED)
    longest = [int(g["row_bytes"][s].max()) for s in range(2)]
    assert longest[1] > longest[0]
    for k in (1, 16, 17):
        budget = k * longest[1]
        sim.set_densities_staging(budget)
        got = written(sim, tmp_path, "rows%d" % k)
        assert got == base, k
        per_section = [-(-ly // min(ly, budget // longest[s])) for s in range(2)]
        assert per_section[1] == -(-ly // k)
        assert sim.densities_stats()[2] == sum(per_section), (k, sim.densities_stats(), per_section)
        assert sim.densities_text() == du.body_of(base[0], case["lx"], ly)
    sim.set_densities_staging(1)       # (less than a row: one row per band)
    assert written(sim, tmp_path, "tiny") == base and sim.densities_stats()[2] == -(-ly // (longest[1] // longest[0])) + ly
    sim.set_densities_staging(0)
    assert written(sim, tmp_path, "again") == base and sim.densities_stats()[2] == 2


MAGNITUDES = (0.5, 12.5, 123.25, 1234.5, 12345.5, 123456.5, 1234567.5, 12345678.5, 123456789.5)


def crafted(sim):
    """f whose velocity sums are exact: all populations of a fluid node zero but f[0] (e = (0, 0)), f[6] (e = (1, 0)) and f[8]
    (e = (0, 1)), so u_x = f[6], u_y = f[8] and the density f[0] + f[6] + f[8] is chosen freely."""
    f, obst = sim.f, sim.obst
    ux = [k / 32 for k in range(-64, 65)]
    for k in (0, 1, 2, 7, 499, 2999):
        t = (k + 0.5) / 1e4
        for v in (t, np.nextafter(t, 0.0), np.nextafter(t, 1.0)):
            ux += [v, -v]
    ux += [-1e-300, -4e-5, -4.9999e-5, -0.0, 0.0]          # just below zero: "-0.0000" (a sum that starts at +0. is never -0.0)
    signed = [s * m for m in MAGNITUDES for s in (1.0, -1.0)]
    pairs = [(a, signed[k % len(signed)]) for k, a in enumerate(ux)] + [(a, b) for a in signed for b in signed]
    excess = [s * 10.0 ** e for e in range(-2, 4) for s in (1.0, -1.0)]   # density - 1: P of one to six integer digits
    nodes = np.argwhere(obst < 0)
    assert len(nodes) >= len(pairs)
    for k, (x, y) in enumerate(nodes):
        a, b = pairs[k % len(pairs)]
        f[x, y, :] = 0.0
        f[x, y, 6], f[x, y, 8] = a, b
        f[x, y, 0] = (1.0 + excess[k % len(excess)]) - a - b
    return f


@pytest.fixture(scope="module")
def crafted_sim(pkg):
    case = dict(lx=64, ly=61, r_mm=np.array([0.6]), x_mm=np.array([1.0]), y_mm=np.array([1.0]))
    sim = make(pkg, case)
    sim.obst_construction()
    assert (sim.obst[1:-1, 1:-1] >= 0).sum() > 0
    return sim


def test_widths_and_ties(pkg, tmp_path, crafted_sim):
    sim = crafted_sim
    sim.f = crafted(sim)
    files = written(sim, tmp_path, "dev")
    assert sim.densities_stats()[3] == 0 and sim.densities_stats()[2] == 2
    f, obst = sim.f, sim.obst
    (tmp_path / "host").mkdir()
    pkg.write_densities_host(str(tmp_path / "host"), du.NFILE, f, obst)
    host = du.read_files(tmp_path / "host")
    du.same_text(files[0], host[0], "host writer")
    du.same_text(files[1], host[1], "host writer")
    want = du.mdg.files(f, obst)
    du.same_text(files[0], want[0].encode(), "restated")
    du.same_text(files[1], want[1].encode(), "restated")
    lines = du.body_of(files[0], 64, 61).split(b"\n")[:-1]
    plines, vlines = lines[:64 * 61], lines[64 * 61:]
    assert {len(l) + 1 for l in vlines} >= set(range(18, 35)), sorted({len(l) + 1 for l in vlines})
    digits = {(l.startswith(b"-"), len(l.lstrip(b"-").split(b".")[0])) for l in plines}
    assert digits >= {(neg, n) for neg in (False, True) for n in range(1, 7)}, sorted(digits)
    assert any(l.startswith(b"-0.0000 ") for l in vlines)
    assert sim.densities_text() == du.body_of(files[0], 64, 61)


def test_host_path_for_what_the_device_refuses(pkg, tmp_path, crafted_sim):
    sim = crafted_sim
    clean = crafted(sim)
    f = clean.copy()
    fluid = np.argwhere(sim.obst < 0)
    (xa, ya), (xb, yb) = fluid[100], fluid[1000]
    f[xa, ya, 3] = np.nan
    f[xb, yb, 6] = 1e12
    sim.f = f
    files = written(sim, tmp_path, "dev")
    assert sim.densities_stats()[2:] == (0, 2)
    (tmp_path / "host").mkdir()
    pkg.write_densities_host(str(tmp_path / "host"), du.NFILE, sim.f, sim.obst)
    host = du.read_files(tmp_path / "host")
    du.same_text(files[0], host[0], "host path")
    du.same_text(files[1], host[1], "host path")
    assert b"nan" in files[0] and b"1000000000000.0000 " in files[0]
    assert sim.densities_text() == du.body_of(files[0], 64, 61) and sim.densities_stats()[2:] == (0, 2)
    sim.f = clean
    written(sim, tmp_path, "clean")
    assert sim.densities_stats()[2:] == (2, 0)


def test_the_run_is_left_alone(pkg, tmp_path):
    case = du.CASES["densities_Lb_131x96"]
    a, b = make(pkg, case), make(pkg, case)
    for sim in (a, b):
        sim.set_change_mask(2)
    for k in range(5):
        a.renderScene(12)
        b.renderScene(12)
        b.write_densities(str(tmp_path), k)
        b.densities_text()
    for what in ("f", "obst", "fhf", "kinematics"):
        assert np.array_equal(getattr(a, what), getattr(b, what)), what
    for sim in (a, b):
        assert sim.dem_chain_recoveries() == 0 and sim.change_mask_stats()[1] == 0
    assert a.dem_chain_paints() == b.dem_chain_paints() and a.obst_stats() == b.obst_stats()
    assert a.nbsteps == b.nbsteps == 60


def test_host_driver_writes_the_densities(pkg, po, tmp_path):
    """`lbmdem <L_b's sample> --steps 24 --densities DIR`: the library's files, numbered with the run's frame counter"""
    name = "densities_Lb_131x96"
    case = du.CASES[name]
    sample = tmp_path / "lb.data"
    po.write_sample(str(sample), case["r_mm"], case["x_mm"], case["y_mm"], comment="#densities Lb")
    (tmp_path / "out").mkdir()
    base = [EXE, str(sample), "--lx", str(case["lx"]), "--ly", str(case["ly"]), "--steps", "24", "--densities", "out"]
    out = subprocess.run(base, capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    names = sorted(os.listdir(tmp_path / "out"))
    assert len(names) == 2 and names[0].startswith("densities") and names[1].startswith("pressure_base"), names
    nfile = int(names[0][len("densities"):-len(".vtk")])
    assert names == ["densities%06d.vtk" % nfile, "pressure_base%06d.dat" % nfile]
    files = tuple(open(tmp_path / "out" / n, "rb").read() for n in names)
    du.is_golden(files, name)
    g = du.golden(name)
    line = "densities: pressure_bytes %d velocity_bytes %d bands 2\n" % (g["row_bytes"][0].sum(), g["row_bytes"][1].sum())
    assert line in out.stderr and out.stderr.index(line) > out.stderr.index("final_density:")
    refused = subprocess.run(base + ["--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert refused.returncode != 0 and "--densities is a single-GPU mode" in refused.stderr
    refused = subprocess.run(base + ["--dry"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert refused.returncode != 0 and "--densities cannot be combined with --dry" in refused.stderr


def test_refusals(pkg, tmp_path):
    import ctypes as C
    import samples
    lx, ly = 256, 200
    r, x1, x2 = samples.to_metres(*samples.row_packing(lx, ly, 600, seed=77))

    def refused(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call(sim)
        assert e.value.code == -1, e.value
        return str(e.value)

    calls = (lambda s: s.write_densities(str(tmp_path), 0), lambda s: s.densities_text())
    strip = pkg.LbmDem(lx, ly, r, x1, x2, strip=(lx // 2, lx), halo=12)
    dist = pkg.LbmDem(lx, ly, r, x1, x2)
    dist.dist_enable()
    for call in calls:
        assert "strip" in refused(strip, call)
        assert "distributed" in refused(dist, call)
    if os.path.exists(pkg.SP_LIB_PATH):
        f32 = pkg.LbmDem(lx, ly, r, x1, x2, precision="f32")
        for call in calls + (lambda s: s.set_densities_staging(0), lambda s: s.densities_stats()):
            assert "single-precision" in refused(f32, call)
    assert os.listdir(tmp_path) == []
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    L, d = sim._L, os.fsencode(str(tmp_path))
    n = C.c_size_t(0)
    few = np.zeros(16, np.uint8)
    assert L.lbmdem_write_densities(sim._h, None, 0) == -1
    assert L.lbmdem_download_densities_text(sim._h, None, 0, None) == -1
    assert L.lbmdem_download_densities_text(sim._h, None, 16, C.byref(n)) == -1
    assert L.lbmdem_download_densities_text(sim._h, few.ctypes.data_as(C.c_void_p), 16, C.byref(n)) == -1 and n.value > 16
    assert L.lbmdem_densities_stats(sim._h, None) == -1
    assert "cannot open" in refused(sim, lambda s: s.write_densities(str(tmp_path / "missing"), 0))
    assert L.lbmdem_write_densities(sim._h, d, 3) == 0 and sorted(os.listdir(tmp_path)) == ["densities000003.vtk", "pressure_base000003.dat"]
