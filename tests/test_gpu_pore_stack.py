"""GPU: the seven pore analyses on ONE handle, in any order (include/lbmdem_hip.h, "Pore space" through "Network pressures"). The
single stages' tests hold every output to its numpy restatement; here the chain is held to the model of tests/pore_stack_util.py
(pinned by tests/test_pore_stack_host.py): after every operation every stage's readers either answer with the restatement of the
compute the model says they belong to -- doubles on the bits, integers by array_equal, rows aligned with the network tables the
handle shows -- or are refused with the stage's own sentence. Downloading readers only; no device view outlives a check."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import clearance_util as cz
import drainage_util as du
import geodesic_util as gu
import netflux_util as fu
import netsolve_util as su
import network_util as nu
import pore_stack_util as ps
import pore_util as pz
import test_gpu_clearance as tc
import test_gpu_drainage as td
import test_gpu_geodesic as tg
import test_gpu_netflux as tf
import test_gpu_netsolve as ts
import test_gpu_network as tn
from test_gpu_pores import shape_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
LX, LY = ps.LX, ps.LY
T, B = ps.T, ps.B
CASES = ps.pair_cases()


def fresh(h):
    """a handle state in which the model prescribes that every reader is refused: behind a fluid step"""
    h.run(ps.step("lbm_step"))
    for stage in ps.STAGES:
        assert h.model.expect(stage).state == "refuses"


@pytest.mark.parametrize("agree", [True, False], ids=["same_merge", "two_merges"])
@pytest.mark.parametrize("first", range(len(CASES)), ids=["%s-%s" % (s, "own" if own else "callers") for s, own in CASES])
def test_ordered_pairs(pkg, first, agree):
    """X, then Y, for every Y: X's readers after X, all seven stages' after Y"""
    r, x, y = shape_scene(LX, LY)
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        h = ps.Harness(pkg, sim, tag="pairs from %s, agree %s:" % (CASES[first], agree))
        for second in CASES:
            fresh(h)
            h.run(ps.pair_op(CASES[first], False, agree))          # (run() holds the compute's own readers to its restatement)
            h.run(ps.pair_op(second, True, agree))
            h.check_all()


def test_two_merges_at_once(pkg):
    """netflux(merge 1, level 1), netsolve(merge -1, level 0), drainage and network(merge 0) in all 24 orders on the handle's map:
    the last answers with its own restatement, every other is refused or answers with the restatement of the parameters it was
    given -- never with rows aligned with another merge's tables (Harness.check: the link count and every lo and hi)"""
    r, x, y = shape_scene(LX, LY)
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        h = ps.Harness(pkg, sim, tag="two merges:")
        for order in itertools.permutations(ps.TWO_MERGES):
            fresh(h)
            for op in order:
                h.run(op)
                h.check_all()
            assert h.model.expect(order[-1].kind).state == "answers"


@pytest.mark.parametrize("seed", ps.SEEDS)
def test_seeded_walks(pkg, seed):
    """40 operations of the full list, steps included, every stage held to the model after each; a failure names the seed, the
    operation and the operations up to it. A twin handle takes the steps and no analysis: what a step reads ends up equal"""
    r, x, y = shape_scene(LX, LY)
    with pkg.LbmDem(LX, LY, r, x, y) as sim, pkg.LbmDem(LX, LY, r, x, y) as twin:
        h = ps.Harness(pkg, sim, twin, tag="walk of seed %d:" % seed)
        # (behind coupled steps: a DEM sub-step alone is refused before the first rebuild of the neighbour lists)
        for op in [ps.step("renderScene")] + ps.walk(seed):
            h.run(op)
            h.check_all()
        h.undisturbed()


# ---- all seven outputs at once ----

MERGE_NETWORK, FLUX, SOLVE, DRAIN, GEO, CONN = 0, (1, 1), (-1, 0, T, 4, B), (T, 4, B), (T, 3, B, 8, 4), 4
PORE_FILES = ("pore_table%06d.dat", "pore_grains%06d.dat", "pores%06d.vtk")
NEW_FILES = PORE_FILES + tc.NEW_FILES + tn.NEW_FILES + td.NEW_FILES + tg.NEW_FILES + tf.NEW_FILES + ts.NEW_FILES
SERIES = dict(pores=pz, clearance=cz, network=nu, drainage=du, geodesic=gu, netflux=fu, netsolve=su)


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    """a packing through run_scene over two DEM events, plain and with all seven analyses' outputs on, their parameters colliding"""
    lx, ly = 61, 59
    r, x, y = shape_scene(lx, ly)
    with_dir, without_dir = tmp_path_factory.mktemp("with"), tmp_path_factory.mktemp("without")
    steps = 8000
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.run_scene(steps, str(without_dir))
        end = {what: getattr(sim, what) for what in ("f", "obst", "kinematics", "fhf")}
    with pkg.LbmDem(lx, ly, r, x, y) as sim:
        sim.set_pores_output(True, CONN, plane=True)
        sim.set_clearance_output(True, plane=True)
        sim.set_network_output(True, merge=MERGE_NETWORK, plane=True)
        sim.set_netflux_output(True, *FLUX)
        sim.set_netsolve_output(True, SOLVE[2], SOLVE[3], SOLVE[4], SOLVE[0], SOLVE[1])
        sim.set_drainage_output(True, *DRAIN, plane=True)
        sim.set_geodesic_output(True, *GEO, plane=True)
        _, res = sim.run_scene(steps, str(with_dir))
        for what in end:
            assert np.array_equal(getattr(sim, what), end[what]), what
        # the last event is the run's last sub-step: the restatements of the state the run ends in
        M, f, n = sim.obst, sim.f, sim.n
        t = sim.nbsteps * sim.config().dt
    W = dict(pores=pz.restate(M, f, n, CONN), clearance=cz.restate(M, n), network=nu.restate(M, n, MERGE_NETWORK),
             drainage=du.restate(M, n, *DRAIN), geodesic=gu.restate(M, n, *GEO), netflux=fu.restate(M, f, n, *FLUX),
             netsolve=su.restate(M, n, SOLVE[2], SOLVE[3], SOLVE[4], SOLVE[0], SOLVE[1]))
    return dict(lx=lx, ly=ly, r=r, x=x, y=y, n=n, with_dir=with_dir, without_dir=without_dir, steps=steps, W=W, t=t, nfile=res["nfile"])


def test_run_scene_with_all_seven_outputs(scene):
    S = scene
    lx, ly, n, W, t, last = S["lx"], S["ly"], S["n"], S["W"], S["t"], S["nfile"]
    others = sorted(os.listdir(S["without_dir"]))
    numbers = sorted({int(name[3:9]) for name in others if name.startswith("DEM") and name.endswith(".dat")})
    assert last in numbers
    new = ["%s.data" % k for k in SERIES] + [p % k for k in numbers for p in NEW_FILES]
    assert len(set(new)) == len(new) and sorted(os.listdir(S["with_dir"])) == sorted(others + new)
    for name in others:
        assert (S["with_dir"] / name).read_bytes() == (S["without_dir"] / name).read_bytes(), name
    events = len((S["with_dir"] / "stats.data").read_text().splitlines())
    assert events == 2
    want = dict(pores=pz.files_bytes(CONN, lx, ly, W["pores"], t, nfile=last, plane=True),
                clearance=cz.files_bytes(lx, ly, n, W["clearance"], t, nfile=last, plane=True),
                network=nu.files_bytes(lx, ly, n, MERGE_NETWORK, W["network"], t, nfile=last, plane=True),
                drainage=du.files_bytes(lx, ly, n, *DRAIN, W["drainage"], W["clearance"]["hist"], t, nfile=last, plane=True),
                geodesic=gu.files_bytes(lx, ly, n, *GEO, W["geodesic"], t, nfile=last, plane=True),
                netflux=fu.files_bytes(lx, ly, n, *FLUX, W["netflux"], t, nfile=last),
                netsolve=su.files_bytes(lx, ly, n, *SOLVE, W["netsolve"], t, nfile=last))
    assert W["network"]["counts"]["bodies"] > W["network"]["counts"]["groups"] >= 1          # (the merges do differ)
    assert sorted(name for files in want.values() for name in files) == sorted(
        ["%s.data" % k for k in SERIES] + [p % last for p in NEW_FILES])
    for stage, files in want.items():
        lines = (S["with_dir"] / ("%s.data" % stage)).read_text().splitlines()
        assert lines[0] + "\n" == SERIES[stage].DATA_HEADER and len(lines) == 1 + events, stage
        assert lines[-1] + "\n" == files.pop("%s.data" % stage).decode(), stage
        for name, data in files.items():
            assert (S["with_dir"] / name).read_bytes() == data, name


def test_host_driver_with_all_seven_outputs(po, scene, tmp_path):
    """`lbmdem <sample>` with every stage's flags together, in a child process: the library run's analysis files, byte for byte"""
    S = scene
    sample = tmp_path / "packing.data"
    po.write_sample(str(sample), S["r"] * 1e3, S["x"] * 1e3, S["y"] * 1e3)
    flags = ["--pores", str(CONN), "--pores-plane", "--clearance", "--clearance-plane", "--network", str(MERGE_NETWORK), "--network-plane",
             "--netflux", str(FLUX[1]), "--netflux-merge", str(FLUX[0]),
             "--netsolve", "T", "--netsolve-to", "B", "--netsolve-band", str(SOLVE[3]), "--netsolve-level", str(SOLVE[1]),
             "--netsolve-merge", str(SOLVE[0]), "--netsolve-rtol", "1e-8", "--netsolve-max-iter", "0",
             "--drainage", "T", "--drainage-to", "B", "--drainage-band", str(DRAIN[1]), "--drainage-plane",
             "--geodesic", "T", "--geodesic-to", "B", "--geodesic-band", str(GEO[1]), "--geodesic-conn", str(GEO[3]),
             "--geodesic-min-d2", str(GEO[4]), "--geodesic-plane"]
    out = subprocess.run([EXE, str(sample), "--lx", str(S["lx"]), "--ly", str(S["ly"]), "--steps", str(S["steps"] + 1)] + flags,
                         capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    plain = set(os.listdir(S["without_dir"]))
    names = [name for name in os.listdir(S["with_dir"]) if name not in plain]
    assert len(names) == len(SERIES) + 2 * len(NEW_FILES)
    for name in names:
        assert (tmp_path / name).read_bytes() == (S["with_dir"] / name).read_bytes(), name
