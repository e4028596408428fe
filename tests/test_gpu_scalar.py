"""GPU: the passive scalar (lbmdem_scalar_*, lbmdem_write_scalar, lbmdem_set_scalar_output; include/lbmdem_hip.h) against its numpy
restatement (tests/scalar_util.py) over the handle's downloads: every population, the record of the fluid nodes and the
concentration exactly equal -- the same bits, no tolerance."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import samples
import scalar_util as su

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "golden", "dem_G6_4000steps")
AB_LIB = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
LX, LY = 256, 200
TAU = 0.8
S_NAMES = sorted(k for k in gu.CASES if k.startswith("S_"))


def g6():
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    return z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def step_and_compare(sim, tau, uv=None, times=1):
    """steps by hand, each against the restatement applied to the downloads taken just before it -> the last (g, was)"""
    for _ in range(times):
        want_g, want_was, want_C = su.expected_step(sim, 1. / tau, uv)
        sim.step_scalar()
        g, was = sim.scalar_state()
        bad = np.argwhere((bits(g) != bits(want_g)).any(2))
        assert len(bad) == 0, (len(bad), bad[:5], [g[tuple(b)] for b in bad[:3]], [want_g[tuple(b)] for b in bad[:3]])
        assert np.array_equal(was, want_was)
        assert same_bits(sim.scalar, want_C)
    return g, was


def neighbours(obst):
    """-> the owners of the four axis neighbours, [4][lx][ly] in the order q = 2, 4, 6, 8; -2 beyond the lattice"""
    return np.stack([su.at(obst, e[0], e[1], -2) for e in su.E[1:]])


def random_field(shape, seed):
    return np.random.default_rng(seed).normal(1.0, 0.5, shape)


@pytest.fixture(scope="module")
def coupled(pkg):
    """the G6 packing on 256 x 200 after five fluid periods and three more sub-steps -> (sim, (ux, uy) of the restatement)"""
    r, x, y = g6()
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        sim.renderScene(5 * sim.cfg.npDEM + 3)
        yield sim, su.planes(sim)


def test_coupled_state(coupled):
    sim, uv = coupled
    obst, n = sim.obst, sim.n
    nb = neighbours(obst)
    fluid = obst == -1
    grain_nb = (nb >= 0) & (nb < n)
    # conditions on the input, not on the code
    assert (fluid & (nb == -1).all(0)).any()                 # four fluid neighbours
    assert (fluid & grain_nb.any(0)).any()                   # next to a grain
    for k in range(4):
        assert (fluid & (nb[k] == n)).any(), k               # next to each of the four walls
    hi, lo = np.where(grain_nb, nb, -1).max(0), np.where(grain_nb, nb, n + 1).min(0)
    assert (fluid & (grain_nb.sum(0) >= 2) & (hi != lo)).any()   # next to two different grains
    assert (np.abs(uv[0][fluid]) > 1e-6).any() and (np.abs(uv[1][fluid]) > 1e-6).any()
    C0 = random_field((LX, LY), 41)
    sim.set_scalar(C0, TAU, automatic=False)
    g, was = sim.scalar_state()
    want_g, want_was = su.initial(C0, obst)
    assert same_bits(g, want_g) and np.array_equal(was, want_was) and same_bits(sim.scalar, su.conc(want_g))
    assert sim.scalar_stats() == {"present": 1, "steps": 0, "hook_steps": 0}
    g3, _ = step_and_compare(sim, TAU, uv, times=3)
    assert sim.scalar_stats() == {"present": 1, "steps": 3, "hook_steps": 0}
    assert (g3[fluid] != g[fluid]).any() and (g3[~fluid] == 0).all()
    # the sums of this state: the restated chains exactly, minimum and maximum included
    got, want = sim.scalar_sums(), su.sums(g3, fluid)
    print("sums", got)
    assert got == want and got["min_C"] < got["max_C"] and got["n_fluid"] == fluid.sum()
    sim.set_scalar(None)
    assert sim.scalar_stats() == {"present": 0, "steps": 0, "hook_steps": 0}
    sim.step_scalar()   # nothing to do


def moving_setup(pkg):
    """G6 plus two grains smaller than a node (reduced radius 0.6 nodes) in open fluid: one centred on a node, which covers that
    node alone -- the only way a node can be uncovered with FOUR eligible neighbours --, one centred between two nodes, which
    covers those two (three eligible neighbours each). No DEM sub-step is made with them: the fluid is stirred by grains given
    velocities, through fluid steps alone."""
    r, x, y = g6()
    cfg = pkg.derive(LX, LY, r)
    # nodes at least three nodes clear of every grain and of the walls, here and ten nodes further up
    xs = (np.arange(LX)[:, None, None] * cfg.dx + cfg.Mgx - x[None, None, :]) / cfg.dx
    ys = (np.arange(LY)[None, :, None] * cfg.dx + cfg.Mby - y[None, None, :]) / cfg.dx
    clear = (np.hypot(xs, ys) - r[None, None, :] / cfg.dx).min(2) > 3.0
    clear[:4] = clear[-4:] = False
    clear[:, :4] = clear[:, -4:] = False
    ok = clear[:-1, :-10] & clear[1:, :-10] & clear[:-1, 10:] & clear[1:, 10:]
    spots = np.argwhere(ok)
    assert len(spots) > 0
    p = spots[0]
    far = spots[np.abs(spots - p).max(1) > 8]
    assert len(far) > 0
    q = far[0]
    tiny = 0.6 * cfg.dx / cfg.phys.reductionR
    r = np.concatenate([r, [tiny, tiny]])
    x = np.concatenate([x, [p[0] * cfg.dx + cfg.Mgx, (q[0] + 0.5) * cfg.dx + cfg.Mgx]])
    y = np.concatenate([y, [p[1] * cfg.dx + cfg.Mby, q[1] * cfg.dx + cfg.Mby]])
    return r, x, y, cfg


def move_grains(k, r, cfg, obst):
    """-> kinematics with grain `a` half a radius aside, grain `b` several radii away, the two small grains ten nodes up"""
    n = len(r)
    inside = [i for i in range(n - 2) if (obst == i).sum() > 40]
    a, b = inside[0], inside[len(inside) // 2]
    k = k.copy()
    k[a, 0] += 0.5 * r[a]
    k[b, 0] += 4.0 * r[b]
    k[b, 1] += 3.0 * r[b]
    k[n - 2, 1] += 10 * cfg.dx
    k[n - 1, 1] += 10 * cfg.dx
    return k, a, b


def moving_classes(before, after, was):
    """conditions on the input of the step after a move -> (covered nodes, eligible-neighbour count of the uncovered nodes)"""
    covered = was & (after != -1)
    uncovered = (after == -1) & ~was
    elig = (after == -1) & was
    cnt = sum(su.at(elig, e[0], e[1], False).astype(int) for e in su.E[1:])
    return covered, uncovered, cnt


def test_moving_grains(pkg):
    r, x, y, cfg = moving_setup(pkg)
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        k = sim.kinematics
        k[:, 3:6] = np.random.default_rng(3).normal(0, 1, (len(k), 3)) * (0.02, 0.02, 5.0)
        sim.kinematics = k
        for _ in range(3):
            sim.lbm_step()
        before = sim.obst
        assert (before == sim.n - 2).sum() == 1 and (before == sim.n - 1).sum() == 2
        sim.set_scalar(random_field((LX, LY), 43), TAU, automatic=False)
        step_and_compare(sim, TAU)
        k2, a, b = move_grains(sim.kinematics, r, cfg, before)
        sim.kinematics = k2
        sim.obst_construction()
        after = sim.obst
        _, was = sim.scalar_state()
        covered, uncovered, cnt = moving_classes(before, after, was)
        assert covered.any() and np.array_equal(was, before == -1)
        for c in (0, 1, 2, 3, 4):
            assert (uncovered & (cnt == c)).any(), c
        filled, want_cnt = su.refill(*sim.scalar_state(), after)
        assert np.array_equal(want_cnt[uncovered], cnt[uncovered])
        g, was2 = step_and_compare(sim, TAU)
        assert np.array_equal(was2, after == -1) and (g[covered] == 0).all()
        # a node of the vacated disc's interior took +0.0 and has only what its neighbours sent it since
        deep = np.argwhere(uncovered & (cnt == 0))
        assert (filled[tuple(deep.T)] == 0).all()
        step_and_compare(sim, TAU, times=2)


@pytest.mark.parametrize("name", S_NAMES)
def test_odd_lattices(pkg, name):
    """the short last window along y, the last rows along x, lattices narrower than a workgroup: one step and the sums"""
    c = gu.CASES[name]
    a = gu.GpuAdapter(pkg, name)
    try:
        a.set_kinematics(gu.mg.shape_initial_kinematics(c))
        sim = a.sim
        sim.renderScene(2 * sim.cfg.npDEM)
        sim.set_scalar(random_field((sim.lx, sim.ly), 7), 0.6, automatic=False)
        g, was = step_and_compare(sim, 0.6)
        assert sim.scalar_sums() == su.sums(g, was) and was.any() and not was.all()
    finally:
        a.sim.close()


def test_sums_of_special_fields(coupled):
    sim, uv = coupled
    fluid = sim.obst == -1
    for C0 in (np.zeros((LX, LY)), np.full((LX, LY), -2.5), random_field((LX, LY), 11) * 1e150):
        sim.set_scalar(C0, 1.0, automatic=False)
        g, was = sim.scalar_state()
        got, want = sim.scalar_sums(), su.sums(g, was)
        assert got == want and got["n_fluid"] == fluid.sum(), (got, want)
    sim.set_scalar(None)
    with pytest.raises(sim_error(sim), match="no scalar is set"):
        sim.scalar_sums()


def sim_error(sim):
    return sys.modules[type(sim).__module__].LbmDemError


def _state(sim):
    return dict(f=sim.f, obst=sim.obst, kinematics=sim.kinematics, fhf=sim.fhf, nbsteps=sim.nbsteps)


def _same_state(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def test_automatic_step_is_the_step_by_hand(pkg):
    r, x, y = g6()
    C0 = random_field((LX, LY), 47)
    with pkg.LbmDem(LX, LY, r, x, y) as a, pkg.LbmDem(LX, LY, r, x, y) as b, pkg.LbmDem(LX, LY, r, x, y) as c:
        period = a.cfg.npDEM
        n = 4 * period + 5
        a.set_scalar(C0, TAU, automatic=True)
        a.renderScene(n)
        assert a.dem_chain_stats()[0] > 0   # the multi-sub-step kernel ran
        b.set_scalar(C0, TAU, automatic=False)
        for s in range(n):
            if s % period == 0:
                b.lbm_step()
                b.step_scalar()
            if s % b.cfg.phys.updateVerlet == 0:
                b.initVerlet()
            b.dem_substep()
        c.renderScene(n)
        (ga, wa), (gb, wb) = a.scalar_state(), b.scalar_state()
        assert same_bits(ga, gb) and np.array_equal(wa, wb) and (ga != su.initial(C0, a.obst)[0]).any()
        assert a.scalar_stats() == {"present": 1, "steps": 5, "hook_steps": 5}
        assert b.scalar_stats() == {"present": 1, "steps": 5, "hook_steps": 0}
        sa, sb, sc = _state(a), _state(b), _state(c)
        assert _same_state(sa, sb) == [] and _same_state(sa, sc) == []   # the scalar changes nothing a step reads
        # automatic == 0: steps leave the field alone
        b.renderScene(period)
        assert same_bits(b.scalar_state()[0], gb) and b.scalar_stats()["steps"] == 5


def test_phases_by_hand(pkg):
    """the fluid step phase by phase, step_scalar() after each forces_fluid, against renderScene with the automatic step"""
    r, x, y = g6()
    C0 = random_field((LX, LY), 53)
    with pkg.LbmDem(LX, LY, r, x, y) as a, pkg.LbmDem(LX, LY, r, x, y) as b:
        period = a.cfg.npDEM
        n = 2 * period + 1
        a.set_scalar(C0, TAU, automatic=True)
        a.renderScene(n)
        b.set_scalar(C0, TAU, automatic=False)
        for s in range(n):
            if s % period == 0:
                b.obst_construction()
                b.collision_streaming()
                b.forces_fluid()
                b.step_scalar()
            if s % b.cfg.phys.updateVerlet == 0:
                b.initVerlet()
            b.dem_substep()
        assert same_bits(a.scalar_state()[0], b.scalar_state()[0]) and _same_state(_state(a), _state(b)) == []
        assert a.scalar_stats()["hook_steps"] == 3 and b.scalar_stats() == {"present": 1, "steps": 3, "hook_steps": 0}


CHILD_PRELUDE = r"""
import os, sys
import numpy as np
root = os.getcwd()
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import __graft_entry__ as ge, samples, scalar_util as su
pkg = ge.load_package()
lx, ly = 256, 160
r, x, y = samples.row_packing(lx, ly, 300, seed=5)
r, x1, x2 = samples.to_metres(r, x, y)
C0 = np.random.default_rng(59).normal(1.0, 0.5, (lx, ly))
"""

RECOVERY_SCRIPT = CHILD_PRELUDE + r"""
a = pkg.LbmDem(lx, ly, r, x1, x2)
b = pkg.LbmDem(lx, ly, r, x1, x2); b.set_dem_chain(0)
k = a.kinematics
k[:, 3:6] = np.random.default_rng(17).normal(0, 1, (len(k), 3)) * (0.05, 0.05, 30.0)
for s in (a, b):
    s.kinematics = k
    s.set_scalar(C0, 0.8, automatic=True)
a.debug_chain_giveup(1)
for n in (37, 1, 12):
    a.renderScene(n); b.renderScene(n)
assert a.dem_chain_stats()[0] > 1 and a.dem_chain_recoveries() == 0, (a.dem_chain_stats(), a.dem_chain_recoveries())
(ga, wa), (gb, wb) = a.scalar_state(), b.scalar_state()            # (the first download settles the handle)
assert a.dem_chain_recoveries() == 1 and b.dem_chain_recoveries() == 0
same = lambda p, q: np.array_equal(p.view(np.uint64), q.view(np.uint64))
assert same(ga, gb) and np.array_equal(wa, wb) and (ga != su.initial(C0, a.obst)[0]).any(), int((ga != gb).any(2).sum())
fluid_steps = sum(1 for s in range(50) if s % a.cfg.npDEM == 0)
want = {"present": 1, "steps": fluid_steps, "hook_steps": fluid_steps}
assert a.scalar_stats() == want and b.scalar_stats() == want, (a.scalar_stats(), b.scalar_stats(), want)
for what in ("f", "obst", "kinematics", "fhf"):
    assert np.array_equal(getattr(a, what), getattr(b, what)), what
print("recovered: scalar", a.scalar_stats())
"""

MEMORY_SCRIPT = CHILD_PRELUDE + r"""
base = pkg.live_memory()
sim = pkg.LbmDem(lx, ly, r, x1, x2)
sim.renderScene(2 * sim.cfg.npDEM + 1)
sim.sync()
held = pkg.live_memory()
sim.step_scalar(); sim.set_scalar(None); sim.set_scalar_output(True); sim.renderScene(sim.cfg.npDEM); sim.set_scalar_output(False)
assert sim.scalar_stats() == {"present": 0, "steps": 0, "hook_steps": 0}
assert pkg.live_memory() == held, (held, pkg.live_memory())          # no scalar: nothing allocated
sim.set_scalar(C0, 0.8)
sy = -(-ly // 16) * 16
with_scalar = pkg.live_memory()
assert with_scalar[0] == held[0] + 4 and with_scalar[1] == held[1] + 81 * lx * sy + 8 * lx * ly, (held, with_scalar)
sim.renderScene(sim.cfg.npDEM)
assert pkg.live_memory() == with_scalar                               # a step takes nothing more
sim.scalar_sums()
assert pkg.live_memory()[0] == with_scalar[0] + 2
sim.set_scalar(C0, 0.7)                                               # the old buffers go, new ones come
assert pkg.live_memory() == with_scalar
sim.set_scalar(None)
assert pkg.live_memory() == held
sim.set_scalar(C0, 0.8)
sim.close()
assert pkg.live_memory() == base, (base, pkg.live_memory())
print("scalar memory ok", held, with_scalar)
"""


def run_child(script, marker):
    assert os.path.exists(AB_LIB), "the experiment build (make -C 2d-lbm-dem_amd/csrc AB=1) is not there"
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=AB_LIB)
    out = subprocess.run([sys.executable, "-c", script], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and marker in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_give_up_recovery_repeats_the_steps_once():
    """as test_give_up_recovery_repeats_the_advances_once (tests/test_gpu_tracers.py): in a process of its own against the
    experiment build, launch 1 of the multi-sub-step kernel gives up on `a` (the library's own cooperative exit, no fault), `b`
    runs without that kernel, both with an automatic scalar and runs of (37, 1, 12): one recovery on `a`, populations and
    counts equal"""
    run_child(RECOVERY_SCRIPT, "recovered: scalar")


def test_no_scalar_no_memory():
    """the experiment build's count of live device blocks and bytes (tests/test_gpu_memory.py): with no scalar nothing is
    allocated, by a step, by a run with the output on; a scalar takes its four blocks of 81 bytes per node of the padded lattice
    and 8 per node of the plane, the sums two more; removing it and closing the handle give everything back"""
    run_child(MEMORY_SCRIPT, "scalar memory ok")


def test_file_and_scene(pkg, tmp_path):
    r, x, y = g6()
    phys = pkg.derive(LX, LY, r).phys
    phys.stepFilm = 60
    C0 = np.zeros((LX, LY))
    C0[100:140, 20:60] = 1.0
    da, dc, dw = tmp_path / "scene", tmp_path / "off", tmp_path / "one"
    for d in (da, dc, dw):
        d.mkdir()
    with pkg.LbmDem(LX, LY, r, x, y, physics=phys) as a, pkg.LbmDem(LX, LY, r, x, y, physics=phys) as c:
        a.set_scalar(C0, TAU)
        a.set_scalar_output(True)
        c.set_scalar(C0, TAU)            # a scalar, but the output off: neither file appears
        _, res = a.run_scene(180, str(da))
        assert res["nfile"] == 3
        c.run_scene(180, str(dc))
        names = ["scalar%06d.vtk" % k for k in range(3)]
        assert sorted(n for n in os.listdir(da) if n.startswith("scalar")) == names   # (no DEM event: no scalar.data)
        others = sorted(n for n in os.listdir(da) if not n.startswith("scalar"))
        assert sorted(os.listdir(dc)) == others and len(others) >= 3
        frames = [n for n in others if n.startswith("fluid_pressure_")]
        assert [n[len("fluid_pressure_"):] for n in frames] == [n[len("scalar"):] for n in names]   # one next to every frame
        for n in others:   # every other file is what a run without the output writes
            assert (dc / n).read_bytes() == (da / n).read_bytes(), n
        assert _same_state(_state(a), _state(c)) == [] and same_bits(a.scalar_state()[0], c.scalar_state()[0])
        # the last frame's file is the present field's
        C = a.scalar
        a.write_scalar(str(dw), 12)
        pkg.write_scalar_files(str(dw), 13, C)
        want = su.file_bytes(C)
        assert (dw / "scalar000012.vtk").read_bytes() == want == (dw / "scalar000013.vtk").read_bytes() == (da / names[2]).read_bytes()
        assert (da / names[0]).read_bytes() != (da / names[2]).read_bytes()
        assert a.scalar_stats()["hook_steps"] == len(range(0, 180, a.cfg.npDEM))
        with pytest.raises(pkg.LbmDemError, match="cannot open"):
            a.write_scalar(str(tmp_path / "not" / "there"), 0)


def test_a_dem_event_appends_a_line_of_scalar_data(pkg, tmp_path):
    """4000 sub-steps: the first DEM event, at the run's last sub-step, so the line is the final state's"""
    r, x, y = g6()
    don, doff = tmp_path / "on", tmp_path / "off"
    don.mkdir(); doff.mkdir()
    C0 = np.zeros((LX, LY))
    C0[100:140, 20:60] = 1.0
    with pkg.LbmDem(LX, LY, r, x, y) as a, pkg.LbmDem(LX, LY, r, x, y) as c:
        a.set_scalar(C0, TAU)
        a.set_scalar_output(True)
        c.set_scalar(C0, TAU)
        a.run_scene(4000, str(don))
        c.run_scene(4000, str(doff))
        assert a.nbsteps == 4000
        g, was = a.scalar_state()
        assert same_bits(g, c.scalar_state()[0])
        want = su.sums(g, was)
        assert a.scalar_sums() == want
        assert sorted(os.listdir(don)) == sorted(os.listdir(doff) + ["scalar.data"]) and "scalar.data" not in os.listdir(doff)
        for name in os.listdir(doff):
            assert (don / name).read_bytes() == (doff / name).read_bytes(), name
        lines = (don / "scalar.data").read_text().splitlines(keepends=True)
        assert lines == [su.DATA_HEADER, su.data_line(4000, want)]
        # the total has drifted only where grains moved: what the sums are for
        print("sum C at the start", float(C0[a.obst == -1].sum()), "after 4000 sub-steps", want["sum_C"])


def test_torch_view_aliases_the_plane(coupled):
    import torch
    sim, uv = coupled
    C0 = random_field((LX, LY), 61)
    sim.set_scalar(C0, TAU, automatic=False)
    t = sim.scalar_tensor()
    sim.sync()
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (LX, LY)
    first = t.cpu().numpy()
    assert same_bits(first, sim.scalar) and same_bits(first, su.conc(su.initial(C0, sim.obst)[0]))
    sim.step_scalar()
    sim.sync()
    assert same_bits(t.cpu().numpy(), first)            # a step does not touch the plane ...
    t2 = sim.scalar_tensor(refresh=False)
    assert t2.data_ptr() == t.data_ptr() and same_bits(t.cpu().numpy(), first)
    sim.scalar_tensor(refresh=True)                      # ... a refresh does, on the handle's stream
    sim.sync()
    now = t.cpu().numpy()   # no other call into the library: the tensor IS the plane
    assert same_bits(now, sim.scalar) and (now != first).any()
    sim.set_scalar(None)
    with pytest.raises(sim_error(sim), match="no scalar is set"):
        sim.scalar_tensor()


WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
NO_SCALAR = ": no scalar is set (lbmdem_scalar_set first)"
DIST = ("the passive scalar is not available with distributed grains (lbmdem_scalar_set(h, NULL, 0, 0) and "
        "lbmdem_set_scalar_output(h, 0) first)")
SP = "the passive scalar is not available in the single-precision build of the library"


def refused(pkg, call, text):
    with pytest.raises(pkg.LbmDemError) as e:
        call()
    assert e.value.code == -1 and text in str(e.value), (text, str(e.value))


def test_refusals(pkg, tmp_path):
    r, x, y = samples.to_metres(*samples.row_packing(LX, LY, 65, seed=29))
    L = pkg.load_library()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = random_field((LX, LY), 5)
    d = os.fsencode(str(tmp_path))

    def calls(s, name):
        """every entry point through its Python method -> [(the C name, the call)]"""
        return [("lbmdem_scalar_set", lambda: s.set_scalar(good, TAU)), ("lbmdem_scalar_step", s.step_scalar),
                ("lbmdem_scalar_download", lambda: s.scalar), ("lbmdem_scalar_download_state", s.scalar_state),
                ("lbmdem_scalar_device", s.scalar_tensor), ("lbmdem_scalar_sums", s.scalar_sums), ("lbmdem_scalar_stats", s.scalar_stats),
                ("lbmdem_write_scalar", lambda: s.write_scalar(str(tmp_path), 0)), ("lbmdem_set_scalar_output", s.set_scalar_output)]

    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        for tau in (0.5, 0.25, -1.0, float("nan"), float("inf")):
            refused(pkg, lambda: sim.set_scalar(good, tau), "lbmdem_scalar_set: the relaxation time must be finite and larger than 0.5 (tau_s = ")
        for bad in (np.nan, np.inf, -np.inf):
            C0 = good.copy()
            C0[17, 33] = bad
            refused(pkg, lambda: sim.set_scalar(C0, TAU), "lbmdem_scalar_set: C[17][33] = %s is not finite" % ("%g" % bad))
        refused(pkg, lambda: sim.set_scalar(good[:-1], TAU), f"set_scalar: a plane of shape ({LX}, {LY})")
        assert sim.scalar_stats()["present"] == 0
        for name, call in calls(sim, "")[2:6] + calls(sim, "")[7:8]:
            if name != "lbmdem_scalar_device":
                refused(pkg, call, name + NO_SCALAR)
        sim.set_scalar(good, TAU)
        g5, w1 = np.zeros((LX, LY, 5)), np.zeros((LX, LY), np.uint8)
        for rc in (L.lbmdem_scalar_download(sim._h, None), L.lbmdem_scalar_download_state(sim._h, None, vp(w1)),
                   L.lbmdem_scalar_download_state(sim._h, vp(g5), None), L.lbmdem_scalar_sums(sim._h, None)):
            assert rc == -1 and L.lbmdem_last_error() == b"null buffer"
        for rc in (L.lbmdem_scalar_device(sim._h, None, 1), L.lbmdem_scalar_stats(sim._h, None)):
            assert rc == -1 and L.lbmdem_last_error() == b"null argument"
        assert L.lbmdem_write_scalar(sim._h, None, 0) == -1 and L.lbmdem_last_error() == b"null directory"
        refused(pkg, lambda: sim.write_scalar(str(tmp_path / "not" / "there"), 0), "cannot open")
        refused(pkg, sim.dist_enable, DIST)     # distributed grains are enabled at a fluid-step boundary
        sim.set_scalar(None)
        sim.set_scalar_output(True)
        refused(pkg, sim.dist_enable, DIST)
        sim.set_scalar_output(False)
        sim.dist_enable()
        for name, call in calls(sim, ""):
            refused(pkg, call, name + WHOLE)
    with pkg.LbmDem(LX, LY, r, x, y, strip=(128, 256), halo=12) as strip:
        for name, call in calls(strip, ""):
            refused(pkg, call, name + WHOLE)
    with pkg.LbmDem(LX, LY, r, x, y, precision="f32") as sp:
        for name, call in calls(sp, ""):
            refused(pkg, call, SP)
    assert os.listdir(tmp_path) == []


def test_checkpoints_do_not_carry_the_scalar(pkg, tmp_path):
    r, x, y = samples.to_metres(*samples.row_packing(LX, LY, 65, seed=29))
    with pkg.LbmDem(LX, LY, r, x, y) as a, pkg.LbmDem(LX, LY, r, x, y) as b:
        a.set_scalar(random_field((LX, LY), 67), TAU)
        a.set_scalar_output(True)
        a.renderScene(30); b.renderScene(30)
        assert a.scalar_stats()["hook_steps"] == len(range(0, 30, a.cfg.npDEM)) > 1
        a.checkpoint_save(str(tmp_path / "a.ckpt")); b.checkpoint_save(str(tmp_path / "b.ckpt"))
        assert (tmp_path / "a.ckpt").read_bytes() == (tmp_path / "b.ckpt").read_bytes()
        assert a.scalar_stats()["present"] == 1   # (saving leaves the scalar alone)
    back = pkg.LbmDem.checkpoint_load(str(tmp_path / "a.ckpt"))
    try:
        assert back.scalar_stats() == {"present": 0, "steps": 0, "hook_steps": 0}
        back.renderScene(12)
        assert back.scalar_stats()["steps"] == 0
        with pytest.raises(pkg.LbmDemError, match="no scalar is set"):
            back.scalar
    finally:
        back.close()
