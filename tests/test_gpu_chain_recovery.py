"""A launch of the multi-sub-step DEM kernel (k_dem_chain) that gives up is undone and the logged calls are replayed one launch
per sub-step (chain_settle_impl, lbmdem_capi.hip). tests/test_gpu_dem_chain.py pins that on a fresh handle with default
settings and nothing but runs behind the launch; here the recovery meets what it has to put back by hand:

  load     a handle loaded from a checkpoint, with a list rebuild queued behind the failed launch (the rebuild's scans do not
           look at the stop word: they must not touch the list the replay runs on -- a loaded handle's per-grain counts were
           never written by a rebuild)
  setter   a setter called between the launch and its discovery: it takes effect at the call, never on the sub-steps asked
           for before it, and the caller's value survives the recovery
  regime   the map updated in place, the change bits verified, vibrating walls (coupled and dry): the rasteriser's and the
           shaker's host state goes back with the launch

Every case: handle `a` (the kernel, one launch made to give up by lbmdem_debug_chain_giveup: the library's own cooperative
exit, no fault) and handle `b` (lbmdem_set_dem_chain(h, 0)) get the same calls and end bit-equal, with one recovery on `a` and
none on `b`; the obst_update and vibration regimes are also held against the CPU oracle, so that the pair cannot be wrong
together. Each case runs in a process of its own against the experiment build (liblbmdem_hip_ab.so).

The scene is samples.row_packing(256, 160, 300): 137 grains in 3 tiles, npDEM = 12, updateVerlet = 100. The checkpoint of the
load cases is taken at sub-step 62, not 60: 60 is a multiple of npDEM = 12 here, and the case wants a sub-step in the middle
of a fluid period. The vibrating cases shake this packing as it is: the left wall travels 0.47 mm, past the packing's margin
of 0.3 mm and into the first grain of every row (grains pressed against the walls beforehand, vib_util.with_wall_grains, make
this packing blow up in the reference's own arithmetic: NaN populations that reach the grains after 375 sub-steps). Every
comparison first checks that the state is finite."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_LIB = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")

CASE_SCRIPT = r"""
import os, sys, tempfile
import numpy as np
root = os.getcwd()
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import __graft_entry__ as ge, samples
pkg = ge.load_package()
kind, name = sys.argv[1], sys.argv[2]
lx, ly = 256, 160
r, x, y = samples.row_packing(lx, ly, 300, seed=5)
r, x1, x2 = samples.to_metres(r, x, y)


def kick(sims, oracle=None, seed=17):
    k = sims[0].kinematics
    k[:, 3:6] = np.random.default_rng(seed).normal(0, 1, (len(k), 3)) * (0.05, 0.05, 30.0)
    for s in sims:
        s.kinematics = k
    if oracle is not None:
        oracle.set_kinematics(k)


def bits(v):
    # the same bits (-0.0 is not 0.0)
    v = np.ascontiguousarray(v)
    return v.view(np.uint64) if v.dtype == np.float64 else v


def same(a, b, coupled, what):
    assert a.nbsteps == b.nbsteps, (what, a.nbsteps, b.nbsteps)
    ka, kb = a.kinematics, b.kinematics          # (the first download settles the handle)
    # a scene that has blown up (the reference's arithmetic can: NaN populations that spread until they reach a grain) would
    # compare the payloads of NaNs: every case stays finite
    assert np.isfinite(ka).all() and np.isfinite(kb).all(), (what, "kinematics not finite", a.nbsteps)
    assert np.array_equal(bits(ka), bits(kb)), (what, "kinematics", a.nbsteps, float(np.abs(ka - kb).max()))
    assert np.array_equal(bits(a.grain_pressure), bits(b.grain_pressure)), (what, "grain_pressure", a.nbsteps)
    if coupled:
        assert np.array_equal(bits(a.fhf), bits(b.fhf)), (what, "fhf", a.nbsteps)
        assert np.array_equal(a.obst, b.obst), (what, "obst", a.nbsteps)
        fa, fb = a.f, b.f
        assert np.isfinite(fa).all() and np.isfinite(fb).all(), (what, "f not finite", a.nbsteps)
        d = np.argwhere(bits(fa) != bits(fb))
        assert len(d) == 0, (what, "f", a.nbsteps, "values that differ", len(d), "max abs", float(np.nanmax(np.abs(fa - fb))),
                             "x", int(d[:, 0].min()), int(d[:, 0].max()), "y", int(d[:, 1].min()), int(d[:, 1].max()))


def same_as_oracle(a, ora, po, coupled, what):
    g = ora.get_grains()
    assert np.array_equal(a.kinematics, g[:, :9]), (what, "kinematics vs oracle", a.nbsteps)
    assert np.array_equal(a.grain_pressure, g[:, po.COL["p"]]), (what, "grain_pressure vs oracle", a.nbsteps)
    if coupled:
        assert np.array_equal(a.fhf, ora.get_fhf()), (what, "fhf vs oracle", a.nbsteps)
        assert np.array_equal(a.obst, ora.get_obst()), (what, "obst vs oracle", a.nbsteps)
        assert np.array_equal(a.f, ora.get_f()), (what, "f vs oracle", a.nbsteps)


def real_contacts(s):
    # the packing has pairs in the list and grains under load: an empty or shifted list would change the result
    cumul, nbrs, _ = s.verlet()
    assert len(nbrs) > 0, len(nbrs)
    assert np.any(s.grain_pressure != 0)


def ends(a, b, giveup):
    assert a.dem_chain_stats()[0] > giveup, (a.dem_chain_stats(), giveup)    # the launch that gives up was made
    assert a.dem_chain_recoveries() == 1, a.dem_chain_recoveries()
    assert b.dem_chain_recoveries() == 0 and b.dem_chain_stats()[:2] == (0, 0)
    real_contacts(a)


if kind == "load":
    coupled = name == "coupled"
    step = (lambda s, n: s.renderScene(n)) if coupled else (lambda s, n: s.run_dem(n))
    u = pkg.LbmDem(lx, ly, r, x1, x2)             # never checkpointed, never interrupted
    kick([u])
    npdem, uv = u.cfg.npDEM, u.cfg.phys.updateVerlet
    s0 = 60 if 60 % npdem else 62
    nxt = (s0 // uv + 1) * uv                      # the next rebuild sub-step
    assert s0 % npdem and s0 % uv and nxt - s0 >= 3 * npdem, (s0, npdem, uv)
    step(u, s0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mid_period.ckpt")
        u.checkpoint_save(path)
        a = pkg.LbmDem.checkpoint_load(path)
        b = pkg.LbmDem.checkpoint_load(path)
    b.set_dem_chain(0)
    giveup = 1 if coupled else 0                   # (launches count from the loaded handle's creation)
    a.debug_chain_giveup(giveup)
    before, across = ((25,), 30) if coupled else ((13, 15), 30)
    for n in before:
        for s in (a, b, u): step(s, n)
    # the failed launch, and one more, lie before the rebuild sub-step ...
    assert a.nbsteps < nxt and a.dem_chain_stats()[0] >= giveup + 2, (a.nbsteps, a.dem_chain_stats())
    for s in (a, b, u): step(s, across)
    # ... and the rebuild has been queued behind it, with nothing but runs in between: nobody has looked yet
    assert a.nbsteps > nxt and a.dem_chain_recoveries() == 0, (a.nbsteps, a.dem_chain_recoveries())
    same(a, b, coupled, "behind the first rebuild")
    assert a.dem_chain_recoveries() == 1
    same(a, u, coupled, "behind the first rebuild, against the uninterrupted handle")
    for s in (a, b, u): step(s, uv)                # across a second rebuild
    assert a.nbsteps > nxt + uv
    same(a, b, coupled, "behind the second rebuild")
    same(a, u, coupled, "behind the second rebuild, against the uninterrupted handle")
    assert u.dem_chain_recoveries() == 0 and u.dem_chain_stats()[0] > a.dem_chain_stats()[0]
    ends(a, b, giveup)

elif kind == "setter":
    a = pkg.LbmDem(lx, ly, r, x1, x2)
    b = pkg.LbmDem(lx, ly, r, x1, x2); b.set_dem_chain(0)
    kick([a, b])
    giveup = 1
    a.debug_chain_giveup(giveup)
    for n in (37, 1):
        a.renderScene(n); b.renderScene(n)
    # the failed launch is pending: made, and nothing since has settled the handle
    assert a.dem_chain_stats()[0] > giveup and a.dem_chain_recoveries() == 0, (a.dem_chain_stats(), a.dem_chain_recoveries())
    n0 = a.nbsteps
    assert n0 == b.nbsteps == 38
    if name == "lid":
        a.set_lid(0.05); b.set_lid(0.05)
    elif name == "force_mode":
        a.set_force_mode(1); b.set_force_mode(1)
    elif name == "nbsteps":
        a.nbsteps = n0 + 1000; b.nbsteps = n0 + 1000
        assert a.nbsteps == n0 + 1000 and b.nbsteps == n0 + 1000, (a.nbsteps, b.nbsteps)
    elif name == "obst_update_on":
        a.set_obst_update(1); b.set_obst_update(1)
    elif name == "obst_update_off":
        a.set_obst_update(0); b.set_obst_update(0)
    elif name == "change_mask_off":
        a.set_change_mask(0); b.set_change_mask(0)
    elif name == "diagnostics":
        a.set_diagnostics(True); b.set_diagnostics(True)
    elif name == "dem_chain_off":
        a.set_dem_chain(0); b.set_dem_chain(0)
    elif name == "dem_chain_keeps_value":
        # the setter's own settle finds the failed launch and switches the kernel off; the caller's value is stored after that
        a.set_dem_chain(64); b.set_dem_chain(0)
    else:
        raise SystemExit("unknown setter " + name)
    assert a.dem_chain_recoveries() == 1, a.dem_chain_recoveries()      # the setter settled the handle
    la = a.dem_chain_stats()[0]
    for i, n in enumerate((12, 200, 95)):
        a.renderScene(n); b.renderScene(n)
        if name == "force_mode" and i == 1:
            a.set_force_mode(0); b.set_force_mode(0)
    same(a, b, True, name)
    if name == "nbsteps":
        assert a.nbsteps == b.nbsteps == n0 + 1000 + 307, (a.nbsteps, b.nbsteps)
    if name == "dem_chain_keeps_value":
        assert a.dem_chain_stats()[0] > la, (a.dem_chain_stats(), la)   # the kernel is back in use, as the caller asked
        la = a.dem_chain_stats()[0]                                      # ... and stays in use: every launch so far is confirmed
        a.renderScene(24); b.renderScene(24)
        assert a.dem_chain_stats()[0] > la, (a.dem_chain_stats(), la)
        same(a, b, True, name + ", and on")
    else:
        assert a.dem_chain_stats()[0] == la, (a.dem_chain_stats(), la)
    ends(a, b, giveup)

elif kind == "regime":
    po = ge.load_oracle()
    po.build_oracle()
    coupled = name != "vibration_dry"
    vib = name.startswith("vibration")
    kw, ora = {}, None
    runs, more = (37, 1, 12, 200, 95), 60
    if vib:
        import vib_util as vu
        total = sum(runs) + more
        dt = pkg.derive(lx, ly, r).dt
        # freq * t sweeps 1.4 rad over the case; the left wall moves some 4 nodes to the right
        phys = vu.physics(pkg, freq=1.4 / (total * dt), amp=4.0 * 1e-4 / (0.5 * total))
        kw = {"physics": phys}
        ora = vu.VibOracle(lx, ly, r, x1, x2, phys=phys)
    elif name == "obst_update":
        ora = po.Oracle(lx, ly, r, x1, x2)
    a = pkg.LbmDem(lx, ly, r, x1, x2, **kw)
    b = pkg.LbmDem(lx, ly, r, x1, x2, **kw); b.set_dem_chain(0)
    for s in (a, b):
        if name == "obst_update": s.set_obst_update(1)
        elif name == "change_mask_verified": s.set_change_mask(2)
        elif vib: s.set_vibration(1)
        else: raise SystemExit("unknown regime " + name)
    kick([a, b], ora)
    step = (lambda s, n: s.renderScene(n)) if coupled else (lambda s, n: s.run_dem(n))
    if ora is None: ora_step = lambda n: None
    elif vib: ora_step = ora.vib_steps if coupled else ora.vib_steps_dry
    else: ora_step = ora.steps
    giveup = 1 if coupled else 0                   # inside the first run of 37 (coupled: its second fluid period)
    a.debug_chain_giveup(giveup)
    mgx0 = a.walls()["Mgx"]
    for i, n in enumerate(runs):
        step(a, n); step(b, n); ora_step(n)
        if i == 0:
            assert a.dem_chain_stats()[0] > giveup, a.dem_chain_stats()
    assert a.dem_chain_recoveries() == 0           # nothing but runs so far
    for lap in ("found at the end of the runs", "and on"):
        same(a, b, coupled, (name, lap))
        if vib:
            wa, wb, wo = a.walls(), b.walls(), ora.walls()
            assert wa == wb and wa == wo, (lap, wa, wb, wo)
        if ora is not None:
            same_as_oracle(a, ora, po, coupled, (name, lap))
        if lap != "and on":
            # the handle takes the kernel back (a new census): runs, rasterisations by their tails and change bits again, from
            # the state the recovery put together
            a.set_dem_chain(128); b.set_dem_chain(0)
            la = a.dem_chain_stats()[0]
            step(a, more); step(b, more); ora_step(more)
            assert a.dem_chain_stats()[0] > la, (a.dem_chain_stats(), la)
    if name == "obst_update":
        assert a.obst_stats()[0] > 0 and b.obst_stats()[0] > 0, (a.obst_stats(), b.obst_stats())   # updates in place ran
    if name == "change_mask_verified":
        assert a.change_mask_stats()[1] == 0 and b.change_mask_stats()[1] == 0, (a.change_mask_stats(), b.change_mask_stats())
    if vib:
        assert a.vibrating and a.walls()["Mgx"] - mgx0 > a.cfg.dx      # the left wall really moved: more than a node
        # ... past the packing's margin (0.3 mm), into the first grain of the rows: the wall the recovery put back is felt
        ka = a.kinematics
        assert int((ka[:, 0] - r - a.walls()["Mgx"] < 0).sum()) >= 3
    ends(a, b, giveup)

else:
    raise SystemExit("unknown case " + kind)
print("recovered:", kind, name, "launches", a.dem_chain_stats()[0], "nbsteps", a.nbsteps)
"""


def run_case(kind, name, lib=AB_LIB):
    """One case in a process of its own against the library `lib` -> (passed, the end of its output)"""
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=lib)
    out = subprocess.run([sys.executable, "-c", CASE_SCRIPT, kind, name], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=300)
    ok = out.returncode == 0 and f"recovered: {kind} {name}" in out.stdout
    return ok, out.stdout[-2000:] + out.stderr[-4000:]


def check_case(kind, name):
    if not os.path.exists(AB_LIB):
        pytest.skip("the experiment build (make -C 2d-lbm-dem_amd/csrc AB=1) is not there")
    ok, text = run_case(kind, name)
    assert ok, text


@pytest.mark.parametrize("mode", ["coupled", "dem"])
def test_a_give_up_on_a_loaded_handle_with_a_rebuild_queued_behind_it(mode):
    """checkpoint at sub-step 62 (mid fluid period, 38 sub-steps before the rebuild at 100), loaded twice; launch 1 (coupled) or 0
    (dem) of the loaded handle gives up, runs go on past sub-step 100, then the first download. Bit-equal to the loaded handle
    without the kernel and to the handle that never stopped, there and behind the rebuild at 200."""
    check_case("load", mode)


SETTERS = ["lid", "force_mode", "nbsteps", "obst_update_on", "obst_update_off", "change_mask_off", "diagnostics",
           "dem_chain_off", "dem_chain_keeps_value"]


@pytest.mark.parametrize("setter", SETTERS)
def test_a_setter_between_the_launch_and_its_discovery_takes_effect_at_the_call(setter):
    """runs (37, 1) with launch 1 giving up, the setter on both handles while that launch is pending, runs (12, 200, 95), download:
    the 38 sub-steps before the setter are repeated with the old setting. set_lid(0.05); set_force_mode(1) and back to 0 two runs
    later; nbsteps + 1000 (read back at once and at the end); set_obst_update(1), (0); set_change_mask(0); set_diagnostics(True);
    set_dem_chain(0); set_dem_chain(64) on the handle that recovers (the kernel is in use again afterwards)."""
    check_case("setter", setter)


@pytest.mark.parametrize("regime", ["obst_update", "change_mask_verified", "vibration", "vibration_dry"])
def test_recovery_in_a_non_default_regime(regime):
    """runs (37, 1, 12, 200, 95) with the give-up inside the first, download, 60 more sub-steps with the kernel back on, download. The map updated in place
    (obst_stats: updates ran; also against the CPU oracle), the change bits verified at every use (nothing hidden), vibrating
    walls coupled and dry (walls compared too; also against the CPU oracle with the reference's vib block)."""
    check_case("regime", regime)
