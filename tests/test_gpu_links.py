"""GPU: the boundary-link export -- act, the effective links with their delta and the six counters of the most recent
rasterisation -- against tests/golden/links_*.npz (the unmodified reference) and the oracle, bit for bit; which map it
describes after a run that has painted for the coming fluid step; that it changes nothing a later step reads; the files of
lbmdem_write_obst and of `lbmdem --dump-geometry`; the refusals."""
import os
import subprocess

import numpy as np
import pytest

import links_util as lu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
LB = "links_Lb_131x96"


def make(pkg, case, **kw):
    r, x1, x2 = lu.mlg.grains_m(case)
    return pkg.LbmDem(case["lx"], case["ly"], r, x1, x2, **kw)


def drive(sim, case):
    """the golden's sequence (make_links_golden.drive) on a handle"""
    if case["steps"]:
        sim.renderScene(case["steps"])
    if case["move_mm"] is not None:
        k = sim.kinematics
        k[:, 0], k[:, 1] = case["move_mm"][0] * 1e-3, case["move_mm"][1] * 1e-3
        sim.kinematics = k
    sim.obst_construction()


def export_of(sim):
    return sim.download_geometry_obst(), sim.download_act(), sim.download_links(), sim.geometry_stats()


def same_export(pkg, got, obst, act, links, census, what):
    assert np.array_equal(got[0], obst), (what, "obst")
    assert np.array_equal(got[1], act), (what, "act", int((got[1] != act).sum()))
    lu.same_links(got[2], links, what)
    assert [got[3][k] for k in pkg.GEOMETRY_COUNTERS] == list(census), (what, got[3], census)


@pytest.mark.parametrize("name", sorted(lu.CASES))
def test_export_is_the_references(pkg, name):
    case, g = lu.CASES[name], lu.golden(name)
    sim = make(pkg, case)
    drive(sim, case)
    same_export(pkg, export_of(sim), g["obst"], g["act"], g["links"], g["census"], name)
    assert np.array_equal(sim.obst, g["obst"])   # (obst_construction has run: the pending map is also what download_obst shows)


@pytest.fixture(scope="module")
def lb_oracle(po):
    """the oracle after L_b's sequence: obst, act, effective links, counters (what travels to the GPU box)"""
    case = lu.CASES[LB]
    r, x1, x2 = lu.mlg.grains_m(case)
    ora = po.Oracle(case["lx"], case["ly"], r, x1, x2)
    lu.mlg.drive(ora, case)
    obst, act = ora.get_obst(), ora.get_act()
    links = lu.mlg.effective_links(obst, act, ora.get_delta(), len(r))
    for a in (obst, act, links):
        a.setflags(write=False)
    return obst, act, links, lu.mlg.census(obst, act, links, len(r))


def test_export_is_the_oracles(pkg, lb_oracle):
    sim = make(pkg, lu.CASES[LB])
    drive(sim, lu.CASES[LB])
    same_export(pkg, export_of(sim), *lb_oracle, "oracle")


@pytest.mark.parametrize("setting", ["obst_update_on", "obst_update_off", "dem_chain_off"])
def test_export_whatever_paints_the_map(pkg, lb_oracle, setting):
    sim = make(pkg, lu.CASES[LB])
    if setting == "dem_chain_off":
        sim.set_dem_chain(0)
    else:
        sim.set_obst_update(setting == "obst_update_on")
    drive(sim, lu.CASES[LB])
    same_export(pkg, export_of(sim), *lb_oracle, setting)


def test_export_describes_the_pending_map_after_a_run(pkg, lb_oracle):
    """run(24) ends where a fluid step begins: the run's last launch has rasterised the discs for it in place, and the export
    shows that map with its centres -- not the map of fluid step 12, whose centres are gone"""
    case = lu.CASES[LB]
    sim = make(pkg, case)
    sim.renderScene(case["steps"])
    assert sim.dem_chain_paints() > 0
    same_export(pkg, export_of(sim), *lb_oracle, "pending")
    sim.renderScene(1)                              # the fluid step consumes it: now the current map, the same export
    same_export(pkg, export_of(sim), *lb_oracle, "consumed")
    assert np.array_equal(sim.obst, lb_oracle[0])


def test_export_leaves_the_run_alone(pkg, tmp_path):
    case = lu.CASES[LB]
    a, b = make(pkg, case), make(pkg, case)
    for sim in (a, b):
        sim.set_change_mask(2)
    for _ in range(5):
        a.renderScene(12)
        b.renderScene(12)
        export_of(b)
        b.write_obst(str(tmp_path))
    for what in ("f", "obst", "fhf", "kinematics"):
        assert np.array_equal(getattr(a, what), getattr(b, what)), what
    for sim in (a, b):
        assert sim.dem_chain_recoveries() == 0 and sim.change_mask_stats()[1] == 0
    assert a.dem_chain_paints() == b.dem_chain_paints() and a.obst_stats() == b.obst_stats()


@pytest.mark.parametrize("name", ["links_La_37x50", "links_Lc_64x61"])
def test_write_obst_writes_the_formatters_files(pkg, tmp_path, name):
    case = lu.CASES[name]
    sim = make(pkg, case)
    drive(sim, case)
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    sim.write_obst(str(tmp_path / "a"))
    pkg.write_obst_files(str(tmp_path / "b"), sim.download_geometry_obst(), sim.download_act(), sim.download_links())
    assert lu.read_files(tmp_path / "a") == lu.read_files(tmp_path / "b")
    g = lu.golden(name)
    assert lu.read_files(tmp_path / "a")[:2] == (lu.map_text(g["obst"]), lu.map_text(g["act"]))
    with pytest.raises(pkg.LbmDemError) as e:
        sim.write_obst(str(tmp_path / "missing"))
    assert e.value.code == -1 and "cannot open" in str(e.value)


def test_host_driver_dumps_the_geometry(pkg, po, tmp_path):
    """`lbmdem <L_a's sample> --steps 0 --dump-geometry DIR`: the reference's own three files of the golden"""
    name = "links_La_37x50"
    case, g = lu.CASES[name], lu.golden(name)
    sample = tmp_path / "la.data"
    po.write_sample(str(sample), case["r_mm"], case["x_mm"], case["y_mm"], comment="#links La")
    (tmp_path / "geo").mkdir()
    base = [EXE, str(sample), "--lx", str(case["lx"]), "--ly", str(case["ly"]), "--steps", "0", "--dump-geometry", "geo"]
    out = subprocess.run(base + ["--run-stats"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    got = lu.read_files(tmp_path / "geo")
    assert got[0] == lu.map_text(g["obst"]) and got[1] == lu.map_text(g["act"])
    assert got[2] == lu.links_text(g["delta_x"], g["delta_y"], g["delta_q"], g["delta_v"])
    c = g["census"]
    line = "geometry: solid_nodes %d active_nodes %d links %d links_near %d links_far %d solid_slots %d\n" % tuple(c)
    assert line in out.stderr and out.stderr.index(line) > out.stderr.index("final_density:")
    refused = subprocess.run(base + ["--gpus", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert refused.returncode != 0 and "--dump-geometry is a single-GPU mode" in refused.stderr


def test_refusals(pkg):
    import samples
    lx, ly = 256, 200
    r, x1, x2 = samples.to_metres(*samples.row_packing(lx, ly, 600, seed=77))

    def refused(sim, call):
        with pytest.raises(pkg.LbmDemError) as e:
            call(sim)
        assert e.value.code == -1, e.value
        return str(e.value)

    calls = (lambda s: s.geometry_stats(), lambda s: s.download_act(), lambda s: s.download_links(),
             lambda s: s.download_geometry_obst(), lambda s: s.write_obst("."))
    strip = pkg.LbmDem(lx, ly, r, x1, x2, strip=(lx // 2, lx), halo=12)
    dist = pkg.LbmDem(lx, ly, r, x1, x2)
    dist.dist_enable()
    for call in calls:
        assert "strip" in refused(strip, call)
        assert "distributed" in refused(dist, call)
    if os.path.exists(pkg.SP_LIB_PATH):
        f32 = pkg.LbmDem(lx, ly, r, x1, x2, precision="f32")
        for call in calls:
            assert "single-precision" in refused(f32, call)
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    import ctypes as C
    n = C.c_long(0)
    few = np.zeros(4, pkg.LINK_DTYPE)
    assert sim._L.lbmdem_download_links(sim._h, few.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == -1 and n.value > 4
    assert sim._L.lbmdem_download_links(sim._h, None, 0, None) == -1
    assert sim._L.lbmdem_download_act(sim._h, None) == -1 and sim._L.lbmdem_geometry_stats(sim._h, None) == -1
    assert sim._L.lbmdem_download_geometry_obst(sim._h, None) == -1
    # a run has painted for a fluid step that never comes: the grains move on, the centres of that picture are gone ...
    sim.renderScene(12)
    assert sim.dem_chain_paints() > 0
    sim.geometry_stats()
    sim.run_dem(1)
    for call in calls:
        assert "rasterisation" in refused(sim, call)
    sim.obst_construction()     # ... until the next rasterisation
    assert sim.geometry_stats()["links"] > 0
