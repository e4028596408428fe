"""GPU: the time-averaged flow statistics (lbmdem_mean_*, lbmdem_write_mean, lbmdem_set_mean_output; include/lbmdem_hip.h) against
their numpy restatement (tests/mean_util.py) over the handle's downloads: every accumulator, count, derived field and profile row
exactly equal -- the same bits, no tolerance."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import mean_util as mu
import samples

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(HERE, "golden", "dem_G6_4000steps")
AB_LIB = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
LX, LY = 256, 200
S_NAMES = sorted(k for k in gu.CASES if k.startswith("S_"))


def g6():
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    return z["r_mm"] * 1e-3, z["x_mm"] * 1e-3, z["y_mm"] * 1e-3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def differing(got, want):
    """the planes of two sets of accumulators (or derived fields) that are not the same bits; a missing plane differs"""
    bad = [k for k in want if k not in got]
    for k in want:
        if k in got:
            same = np.array_equal(got[k], want[k]) if want[k].dtype == np.uint32 else same_bits(got[k], want[k])
            if not same:
                bad.append(k)
    return bad + [k for k in got if k not in want]


def moving_setup(pkg):
    """tests/test_gpu_scalar.py's: G6 plus two grains smaller than a node (reduced radius 0.6 nodes) in open fluid, one centred on
    a node, one between two nodes. No DEM sub-step is made with them: the fluid is stirred by grains given velocities."""
    r, x, y = g6()
    cfg = pkg.derive(LX, LY, r)
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
    return k


@pytest.fixture(scope="module")
def hand(pkg):
    """three samples by hand on a coupled state whose grains move between them (a fluid step, a change of the kinematics and
    obst_construction between two samples), the restatement applied to the downloads taken just before each -> dict(sim: the
    handle with that window open, want: the restated window, bad: per sample the planes that differed, F: the three inputs)"""
    r, x, y, cfg = moving_setup(pkg)
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        k = sim.kinematics
        k[:, 3:6] = np.random.default_rng(3).normal(0, 1, (len(k), 3)) * (0.02, 0.02, 5.0)
        sim.kinematics = k
        for _ in range(3):
            sim.lbm_step()
        sim.begin_mean(mu.ALL, 0)
        want = mu.window((LX, LY))
        bad, inputs = [], []
        k0 = sim.kinematics
        for s in range(3):
            if s > 0:
                sim.lbm_step()
                if s == 1:
                    sim.kinematics = move_grains(sim.kinematics, r, cfg, sim.obst)
                else:   # back to where they were: nodes change class a second time
                    k = sim.kinematics
                    k[:, 0:2] = k0[:, 0:2]
                    sim.kinematics = k
                sim.obst_construction()
            F = mu.state(sim)
            inputs.append(F)
            mu.sample(want, F)
            sim.sample_mean()
            bad.append(differing(sim.mean_accumulators(), want))
        yield dict(sim=sim, want=want, bad=bad, F=inputs, samples=3)


def test_samples_by_hand_with_moving_grains(hand):
    sim, F = hand["sim"], hand["F"]
    assert hand["bad"] == [[], [], []]
    assert sim.mean_stats() == dict(present=1, mask=mu.ALL, samples=3, hook_steps=0, bytes=LX * 208 * (8 + 8 * 11))
    # conditions on the input, not on the code
    nfl = sum(f["fluid"].astype(int) for f in F)
    ngr = sum(f["grain"].astype(int) for f in F)
    assert (nfl == 3).any()                                # fluid in all three samples
    assert ((nfl > 0) & (ngr > 0)).any()                   # fluid in some, a grain's in others
    assert (ngr == 3).any()                                # a grain's throughout
    assert ((nfl == 0) & (ngr == 0)).any() and (nfl + ngr)[0, :].max() == 0 and (nfl + ngr)[:, -1].max() == 0   # walls: both counts 0
    assert all((np.abs(f["uy"][f["fluid"]]) > 1e-6).any() and (np.abs(f["uy"][f["grain"]]) > 1e-6).any() for f in F)
    assert any(not np.array_equal(F[0]["grain"], f["grain"]) for f in F[1:])
    acc = sim.mean_accumulators()
    assert np.array_equal(acc["n_fluid"], nfl) and np.array_equal(acc["n_grain"], ngr)
    assert acc["Sdiss"][nfl == 3].min() >= 0 and acc["Sdiss"][nfl == 3].max() > 0 and (acc["Sgux"][ngr == 0] == 0).all() and (acc["Sux"][nfl == 0] == 0).all()


def test_derived_fields_and_profile(hand, pkg):
    import torch
    sim, want = hand["sim"], hand["want"]
    D = mu.derived(want, 3)
    got = sim.mean_fields()
    assert list(got) == list(mu.FIELDS) and differing(got, D) == []
    assert (D["phi"] + D["solid"] <= 1.0).all() and (D["rxx"] != 0).any() and (D["vrho"] != 0).any() and (D["guy"] != 0).any()
    P = sim.mean_profile()
    assert same_bits(P, mu.profile(D, want["n_fluid"])) and (P[13] > 0).any()
    # a subset comes in ascending bit order
    sub = sim.mean_fields(pkg.MEANF_GUY | pkg.MEANF_PHI | pkg.MEANF_RXY)
    assert list(sub) == ["phi", "rxy", "guy"] and differing(sub, {k: D[k] for k in sub}) == []
    # the torch route: the same bytes
    t = torch.empty((13, LX, LY), dtype=torch.float64, device=f"cuda:{sim.cfg.device}")
    sim.mean_fields_into(pkg.MEANF_ALL, t)
    sim.sync()
    assert same_bits(t.cpu().numpy(), np.stack([got[k] for k in mu.FIELDS]))
    dev = sim.mean_fields(pkg.MEANF_UX | pkg.MEANF_VRHO, device=True)
    sim.sync()
    assert same_bits(dev["mux"].cpu().numpy(), D["mux"]) and same_bits(dev["vrho"].cpu().numpy(), D["vrho"])
    with pytest.raises(pkg.LbmDemError, match="the planes are %d doubles, the buffer holds %d" % (13 * LX * LY, LX * LY)):
        sim.mean_fields_into(pkg.MEANF_ALL, t[0])


def test_fields_outside_the_mask_and_empty_windows_are_refused(pkg):
    r, x, y = samples.to_metres(*samples.row_packing(LX, LY, 65, seed=29))
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        k = sim.kinematics
        k[:, 3:6] = np.random.default_rng(9).normal(0, 1, (len(k), 3)) * (0.02, 0.02, 5.0)
        sim.kinematics = k
        for _ in range(3):
            sim.lbm_step()
        sim.begin_mean(pkg.MEAN_U | pkg.MEAN_GRAIN, 0)
        for call in (sim.mean_fields, sim.mean_profile, lambda: sim.write_mean(".", 0)):
            with pytest.raises(pkg.LbmDemError, match="no sample has been taken"):
                call()
        sim.sample_mean()
        for fmask, name, needs in ((pkg.MEANF_RXY, "rxy", 3), (pkg.MEANF_UX | pkg.MEANF_VRHO, "vrho", 4), (pkg.MEANF_ALL, "rxx", 3),
                                   (pkg.MEANF_GDOT, "mgdot", 8)):
            with pytest.raises(pkg.LbmDemError) as e:
                sim.mean_fields(fmask)
            assert f"lbmdem_mean_fields: the field {name} needs accumulators that are not in the window's mask 17 (it needs {needs})" in str(e.value)
        got = sim.mean_fields(pkg.MEANF_PHI | pkg.MEANF_UY | pkg.MEANF_GUX)
        want = mu.window((LX, LY), mu.U | mu.GRAIN)
        mu.sample(want, mu.state(sim))
        D = mu.derived(want, 1)
        assert differing(got, {k: D[k] for k in ("phi", "muy", "gux")}) == []
        # the profile of a window without some accumulators: rows of +0.0 there
        P = sim.mean_profile()
        assert same_bits(P, mu.profile(D, want["n_fluid"])) and not P[4:11].any() and P[3].any()
        sim.end_mean()
        assert sim.mean_stats() == dict(present=0, mask=0, samples=0, hook_steps=0, bytes=0)
        for call in (sim.sample_mean, sim.reset_mean, sim.mean_accumulators, sim.mean_fields, sim.mean_profile):
            with pytest.raises(pkg.LbmDemError, match=r"no window is open \(lbmdem_mean_begin first\)"):
                call()
        sim.end_mean()   # nothing to do


def _state(sim):
    return dict(f=sim.f, obst=sim.obst, kinematics=sim.kinematics, fhf=sim.fhf, nbsteps=sim.nbsteps)


def _same_state(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])]


def by_hand(sim, n, sample_at, phases=False):
    """n x renderScene with the fluid step's parts called one by one; sample_mean() behind the fluid steps whose number (1, 2, ..
    counted from `first`) sample_at says"""
    period = sim.cfg.npDEM
    k = by_hand.count.get(id(sim), 0)
    for _ in range(n):
        s = sim.nbsteps
        if s % period == 0:
            if phases:
                sim.obst_construction()
                sim.collision_streaming()
                sim.forces_fluid()
            else:
                sim.lbm_step()
            k += 1
            if sample_at(k):
                sim.sample_mean()
        if s % sim.cfg.phys.updateVerlet == 0:
            sim.initVerlet()
        sim.dem_substep()
    by_hand.count[id(sim)] = k


by_hand.count = {}


def test_the_hook_is_the_sample_by_hand(pkg):
    r, x, y = g6()
    new = lambda: pkg.LbmDem(LX, LY, r, x, y)
    with new() as a, new() as b, new() as c, new() as d, new() as e:
        by_hand.count.clear()
        period = a.cfg.npDEM
        n = 4 * period + 5
        a.begin_mean(mu.ALL, 1)
        a.renderScene(n)
        assert a.dem_chain_stats()[0] > 0   # the multi-sub-step kernel ran
        b.begin_mean(mu.ALL, 0)
        by_hand(b, n, lambda k: True, phases=True)
        c.renderScene(n)
        A, B = a.mean_accumulators(), b.mean_accumulators()
        assert differing(A, B) == [] and (A["Sux"] != 0).any() and A["n_fluid"].max() == 5
        assert a.mean_stats() == dict(present=1, mask=31, samples=5, hook_steps=5, bytes=LX * 208 * 96)
        assert b.mean_stats() == dict(present=1, mask=31, samples=5, hook_steps=0, bytes=LX * 208 * 96)
        sa, sb, sc = _state(a), _state(b), _state(c)
        assert _same_state(sa, sb) == [] and _same_state(sa, sc) == []   # a window changes nothing a step reads
        # every second fluid step
        d.begin_mean(mu.U | mu.RHO, 2)
        d.renderScene(n)
        e.begin_mean(mu.U | mu.RHO, 0)
        by_hand(e, n, lambda k: k % 2 == 0)
        assert d.mean_stats() == dict(present=1, mask=5, samples=2, hook_steps=5, bytes=LX * 208 * 40)
        Dd, De = d.mean_accumulators(), e.mean_accumulators()
        assert sorted(Dd) == ["Srho", "Srho2", "Sux", "Suy", "n_fluid", "n_grain"] and differing(Dd, De) == [] and Dd["n_fluid"].max() == 2
        # a reset zeroes the window and keeps the phase: the sixth fluid step is sampled, the seventh is not
        d.reset_mean()
        e.reset_mean()
        assert d.mean_stats() == dict(present=1, mask=5, samples=0, hook_steps=1, bytes=LX * 208 * 40)
        Z = d.mean_accumulators()
        assert all(not v.any() for v in Z.values()) and all(not np.signbit(Z[k]).any() for k in ("Sux", "Suy", "Srho", "Srho2"))
        d.renderScene(2 * period)
        by_hand(e, 2 * period, lambda k: k % 2 == 0)
        assert d.mean_stats()["samples"] == 1 and d.mean_stats()["hook_steps"] == 3
        Dd, De = d.mean_accumulators(), e.mean_accumulators()
        assert differing(Dd, De) == [] and Dd["n_fluid"].max() == 1 and _same_state(_state(d), _state(e)) == []


@pytest.mark.parametrize("name", S_NAMES)
def test_odd_lattices(pkg, name):
    """the short last window along y, the last segment along x, lattices narrower than a workgroup: two samples a fluid step
    apart, then accumulators, derived fields and profile"""
    c = gu.CASES[name]
    a = gu.GpuAdapter(pkg, name)
    try:
        a.set_kinematics(gu.mg.shape_initial_kinematics(c))
        sim = a.sim
        sim.renderScene(2 * sim.cfg.npDEM)
        sim.begin_mean(mu.ALL, 0)
        want = mu.window((sim.lx, sim.ly))
        for _ in range(2):
            sim.lbm_step()
            mu.sample(want, mu.state(sim))
            sim.sample_mean()
        assert differing(sim.mean_accumulators(), want) == []
        D = mu.derived(want, 2)
        assert differing(sim.mean_fields(), D) == [] and same_bits(sim.mean_profile(), mu.profile(D, want["n_fluid"]))
        assert (want["n_fluid"] == 2).any() and (want["n_grain"] == 2).any()
    finally:
        a.sim.close()


CHILD_PRELUDE = r"""
import os, sys
import numpy as np
root = os.getcwd()
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import __graft_entry__ as ge, samples, mean_util as mu
pkg = ge.load_package()
lx, ly = 256, 160
r, x, y = samples.row_packing(lx, ly, 300, seed=5)
r, x1, x2 = samples.to_metres(r, x, y)
same = lambda p, q: p.dtype == q.dtype and np.array_equal(p.view(np.uint32 if p.dtype == np.uint32 else np.uint64), q.view(np.uint32 if q.dtype == np.uint32 else np.uint64))
"""

RECOVERY_SCRIPT = CHILD_PRELUDE + r"""
a = pkg.LbmDem(lx, ly, r, x1, x2)
b = pkg.LbmDem(lx, ly, r, x1, x2); b.set_dem_chain(0)
k = a.kinematics
k[:, 3:6] = np.random.default_rng(17).normal(0, 1, (len(k), 3)) * (0.05, 0.05, 30.0)
for s in (a, b):
    s.kinematics = k
    s.begin_mean(mu.ALL, 1)
a.debug_chain_giveup(1)
for n in (37, 1, 12):
    a.renderScene(n); b.renderScene(n)
assert a.dem_chain_stats()[0] > 1 and a.dem_chain_recoveries() == 0, (a.dem_chain_stats(), a.dem_chain_recoveries())
A, B = a.mean_accumulators(), b.mean_accumulators()            # (the first download settles the handle)
assert a.dem_chain_recoveries() == 1 and b.dem_chain_recoveries() == 0
assert sorted(A) == sorted(B) and all(same(A[n], B[n]) for n in A), [n for n in A if not same(A[n], B[n])]
fluid_steps = sum(1 for s in range(50) if s % a.cfg.npDEM == 0)
assert fluid_steps > 2 and A["n_fluid"].max() == fluid_steps and (A["Sux"] != 0).any()      # every sample made once
want = dict(present=1, mask=31, samples=fluid_steps, hook_steps=fluid_steps, bytes=lx * ly * 96)
assert a.mean_stats() == want and b.mean_stats() == want, (a.mean_stats(), b.mean_stats(), want)
for what in ("f", "obst", "kinematics", "fhf"):
    assert np.array_equal(getattr(a, what), getattr(b, what)), what
print("recovered: mean", a.mean_stats())
"""

MEMORY_SCRIPT = CHILD_PRELUDE + r"""
base = pkg.live_memory()
sim = pkg.LbmDem(lx, ly, r, x1, x2)
sim.renderScene(2 * sim.cfg.npDEM + 1)
sim.sync()
held = pkg.live_memory()
sim.set_mean_output(0); sim.renderScene(sim.cfg.npDEM); sim.end_mean()
assert sim.mean_stats() == dict(present=0, mask=0, samples=0, hook_steps=0, bytes=0)
assert pkg.live_memory() == held, (held, pkg.live_memory())          # no window: nothing allocated
plane = lx * ly                                                       # (ly = 160 is a multiple of 16: the pitch is ly)
sim.begin_mean(mu.ALL, 0)
assert pkg.live_memory() == (held[0] + 2, held[1] + plane * 96) and sim.mean_stats()["bytes"] == plane * 96
sim.sample_mean(); sim.sample_mean()
ALL = sim.mean_accumulators()
assert pkg.live_memory() == (held[0] + 2, held[1] + plane * 96)      # sampling and the download take nothing more
for bit, group in enumerate(mu.PLANES):
    sim.begin_mean(1 << bit, 0)                                       # another mask: the old planes go, the new ones come
    size = plane * (8 + 8 * len(group))
    assert pkg.live_memory() == (held[0] + 2, held[1] + size), (bit, held, pkg.live_memory())
    assert sim.mean_stats() == dict(present=1, mask=1 << bit, samples=0, hook_steps=0, bytes=size)
    sim.sample_mean(); sim.sample_mean()
    got = sim.mean_accumulators()
    assert sorted(got) == sorted(group + ("n_fluid", "n_grain")), (bit, sorted(got))
    assert all(same(got[n], ALL[n]) for n in got), (bit, [n for n in got if not same(got[n], ALL[n])])
assert (ALL["Sux"] != 0).any() and (ALL["Sgux"] != 0).any() and ALL["n_fluid"].max() == 2 and ALL["n_grain"].max() == 2
sim.mean_fields(pkg.MEANF_PHI)                                        # the readers' scratch: one more block
assert pkg.live_memory()[0] == held[0] + 3
sim.end_mean()
assert pkg.live_memory() == held                                      # everything back
sim.begin_mean(mu.ALL, 1)
sim.renderScene(sim.cfg.npDEM)
assert pkg.live_memory() == (held[0] + 2, held[1] + plane * 96) and sim.mean_stats()["samples"] == 1
sim.close()
assert pkg.live_memory() == base, (base, pkg.live_memory())
print("mean memory ok", held)
"""


def run_child(script, marker):
    assert os.path.exists(AB_LIB), "the experiment build (make -C 2d-lbm-dem_amd/csrc AB=1) is not there"
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=AB_LIB)
    out = subprocess.run([sys.executable, "-c", script], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and marker in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_mask_subsets_hold_the_same_planes_and_only_those():
    """in a process of its own against the experiment build, which counts its live device blocks and bytes
    (tests/test_gpu_memory.py): every single-bit mask gives the planes ALL gives; a window is two blocks of 8 bytes of counts and
    8 per selected plane for every node of the padded lattice, which is what mean_stats says; the readers' scratch is one more
    block; end_mean and closing the handle give everything back; without a window nothing is allocated"""
    run_child(MEMORY_SCRIPT, "mean memory ok")


def test_give_up_recovery_repeats_the_samples_once():
    """as test_give_up_recovery_repeats_the_steps_once (tests/test_gpu_scalar.py): in a process of its own against the
    experiment build, launch 1 of the multi-sub-step kernel gives up on `a` (the library's own cooperative exit, no fault), `b`
    runs without that kernel, both with a hooked window and runs of (37, 1, 12): one recovery on `a`, accumulators and counts
    equal, every node's count at most the number of fluid steps"""
    run_child(RECOVERY_SCRIPT, "recovered: mean")


def profile_samples(path):
    lines = path.read_text().splitlines()
    assert lines[0] + "\n" == mu.PROFILE_HEADER and len(lines) == LY + 1
    counts = {l.split()[1] for l in lines[1:]}
    assert len(counts) == 1
    return int(counts.pop())


def test_files_and_scene(pkg, tmp_path):
    r, x, y = g6()
    phys = pkg.derive(LX, LY, r).phys
    phys.stepFilm = 60
    da, db, dc, dw = (tmp_path / n for n in ("scene", "hand", "off", "one"))
    for d in (da, db, dc, dw):
        d.mkdir()
    new = lambda: pkg.LbmDem(LX, LY, r, x, y, physics=phys)
    with new() as a, new() as b, new() as c:
        period = a.cfg.npDEM
        a.set_mean_output(mu.ALL, 1)
        lines_a, res = a.run_scene(120, str(da))
        assert res["nfile"] == 2
        lines_c, _ = c.run_scene(120, str(dc))
        names = sorted(["mean%06d.vtk" % k for k in range(2)] + ["mean_profile%06d.dat" % k for k in range(2)])
        assert sorted(n for n in os.listdir(da) if n.startswith("mean")) == names
        others = sorted(n for n in os.listdir(da) if not n.startswith("mean"))
        assert sorted(os.listdir(dc)) == others and len(others) >= 2
        for n in others:   # every other file, and the console, are what a run without the setting gives
            assert (dc / n).read_bytes() == (da / n).read_bytes(), n
        strip_clock = lambda ls: [l[:l.index(" Time ") + 6] if l.startswith("steps ") else l for l in ls]
        assert strip_clock(lines_a) == strip_clock(lines_c) and len(lines_a) > 0
        assert _same_state(_state(a), _state(c)) == []
        # each window holds the fluid steps since the event before
        for k in range(2):
            assert profile_samples(da / ("mean_profile%06d.dat" % k)) == len([s for s in range(60 * k, 60 * k + 60) if s % period == 0]) > 1
        assert a.mean_stats() == dict(present=1, mask=31, samples=0, hook_steps=0, bytes=LX * 208 * 96)   # (reset at the last event)
        # a second handle stepped by hand on the same cadence
        b.begin_mean(mu.ALL, 1)
        b.renderScene(60)
        b.write_mean(str(db), 0)
        b.reset_mean()
        b.renderScene(60)
        b.write_mean(str(db), 1)
        for n in names:
            assert (db / n).read_bytes() == (da / n).read_bytes(), n
        assert (da / names[0]).read_bytes() != (da / names[1]).read_bytes()
        # the library's file is the host writer's over the downloads, which is the file assembled here
        D, P, ns = b.mean_fields(), b.mean_profile(), b.mean_stats()["samples"]
        seven = [D[k] for k in ("phi", "mux", "muy", "rxx", "rxy", "ryy", "mrho")]
        pkg.write_mean_files(str(dw), 13, ns, *seven, P)
        assert (dw / "mean000013.vtk").read_bytes() == (da / "mean000001.vtk").read_bytes() == mu.file_bytes(*seven)
        assert (dw / "mean_profile000013.dat").read_bytes() == (da / "mean_profile000001.dat").read_bytes() == mu.profile_text(P, ns, LX)
        acc = b.mean_accumulators()
        assert differing(D, mu.derived(acc, ns)) == [] and (D["rxx"] != 0).any()
        # a window without the velocity: those planes of the file are +0.0
        b.begin_mean(mu.RHO, 0)
        b.sample_mean()
        b.write_mean(str(dw), 14)
        Dr = b.mean_fields(pkg.MEANF_PHI | pkg.MEANF_RHO)
        zero = np.zeros((LX, LY))
        assert (dw / "mean000014.vtk").read_bytes() == mu.file_bytes(Dr["phi"], zero, zero, zero, zero, zero, Dr["mrho"])
        with pytest.raises(pkg.LbmDemError, match="cannot open"):
            b.write_mean(str(tmp_path / "not" / "there"), 0)
        # the setting off again: a run writes no such file and opens no window
        a.set_mean_output(0)
        a.end_mean()
        a.run_scene(60, str(da))
        assert sorted(n for n in os.listdir(da) if n.startswith("mean")) == names and a.mean_stats()["present"] == 0


WHOLE = " needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)"
DIST = ("time averaging is not available with distributed grains (lbmdem_mean_end(h) and lbmdem_set_mean_output(h, 0, 0) "
        "first)")
SP = "time averaging is not available in the single-precision build of the library"


def refused(pkg, call, text):
    with pytest.raises(pkg.LbmDemError) as e:
        call()
    assert e.value.code == -1 and text in str(e.value), (text, str(e.value))


def test_refusals(pkg, tmp_path):
    r, x, y = samples.to_metres(*samples.row_packing(LX, LY, 65, seed=29))
    L = pkg.load_library()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    d = os.fsencode(str(tmp_path))

    def calls(s):
        """every entry point through its Python method -> [(the C name, the call)]"""
        return [("lbmdem_mean_begin", s.begin_mean), ("lbmdem_mean_sample", s.sample_mean), ("lbmdem_mean_reset", s.reset_mean),
                ("lbmdem_mean_end", s.end_mean), ("lbmdem_mean_stats", s.mean_stats),
                ("lbmdem_mean_fields", s.mean_fields), ("lbmdem_mean_fields_device", lambda: s.mean_fields(device=True)),
                ("lbmdem_mean_profile", s.mean_profile), ("lbmdem_write_mean", lambda: s.write_mean(str(tmp_path), 0)),
                ("lbmdem_set_mean_output", s.set_mean_output)]

    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        for mask in (0, -1, 32, 63):
            refused(pkg, lambda: sim.begin_mean(mask, 1), "lbmdem_mean_begin: bad mask %d" % mask)
        for mask in (-1, 32):
            refused(pkg, lambda: sim.set_mean_output(mask, 1), "lbmdem_set_mean_output: bad mask %d" % mask)
        refused(pkg, lambda: sim.begin_mean(31, -1), "lbmdem_mean_begin: every = -1 is negative")
        refused(pkg, lambda: sim.set_mean_output(31, 0), "lbmdem_set_mean_output: every = 0, the scene samples every k-th fluid step, k >= 1")
        assert sim.mean_stats()["present"] == 0
        sim.begin_mean(31, 1)
        sim.lbm_step()
        for fmask in (0, -4, 8192):
            with pytest.raises(pkg.LbmDemError, match="bad field mask"):
                sim.mean_fields(fmask)
            n = ctypes.c_long(0)
            one = np.zeros(4)
            assert L.lbmdem_mean_fields(sim._h, fmask, vp(one), 4, ctypes.byref(n)) == -1
            assert L.lbmdem_last_error() == b"lbmdem_mean_fields: bad mask %d" % fmask
            assert L.lbmdem_mean_fields_device(sim._h, fmask, vp(one), 4) == -1
        n = ctypes.c_long(-1)
        big = np.zeros(LX * LY)
        cnt = np.zeros((LX, LY), np.uint32)
        for rc in (L.lbmdem_mean_download(sim._h, None, vp(cnt), vp(cnt), 5, ctypes.byref(n)),
                   L.lbmdem_mean_download(sim._h, vp(big), None, vp(cnt), 5, ctypes.byref(n)),
                   L.lbmdem_mean_download(sim._h, vp(big), vp(cnt), vp(cnt), 5, None),
                   L.lbmdem_mean_fields(sim._h, 1, None, 5, ctypes.byref(n)), L.lbmdem_mean_fields(sim._h, 1, vp(big), 5, None),
                   L.lbmdem_mean_fields_device(sim._h, 1, None, 5), L.lbmdem_mean_profile(sim._h, None, 14 * LY)):
            assert rc == -1 and L.lbmdem_last_error() == b"null buffer"
        assert L.lbmdem_mean_stats(sim._h, None) == -1 and L.lbmdem_last_error() == b"null argument"
        assert L.lbmdem_write_mean(sim._h, None, 0) == -1 and L.lbmdem_last_error() == b"null directory"
        # short buffers, the count reported
        assert L.lbmdem_mean_download(sim._h, vp(big), vp(cnt), vp(cnt), LX * LY, ctypes.byref(n)) == -1 and n.value == 11 * LX * LY
        assert b"lbmdem_mean_download: the planes are %d doubles, the buffer holds %d" % (11 * LX * LY, LX * LY) == L.lbmdem_last_error()
        assert L.lbmdem_mean_fields(sim._h, 3, vp(big), LX * LY, ctypes.byref(n)) == -1 and n.value == 2 * LX * LY
        assert L.lbmdem_mean_fields(sim._h, 7, None, 0, ctypes.byref(n)) == 0 and n.value == 3 * LX * LY
        assert L.lbmdem_mean_profile(sim._h, vp(big), 14 * LY - 1) == -1
        assert b"lbmdem_mean_profile: the profile is %d doubles, the buffer holds %d" % (14 * LY, 14 * LY - 1) == L.lbmdem_last_error()
        refused(pkg, lambda: sim.write_mean(str(tmp_path / "not" / "there"), 0), "cannot open")
        refused(pkg, sim.dist_enable, DIST)     # distributed grains are enabled at a fluid-step boundary
        sim.end_mean()
        sim.set_mean_output(31, 2)
        refused(pkg, sim.dist_enable, DIST)
        sim.set_mean_output(0)
        sim.dist_enable()
        for name, call in calls(sim):
            refused(pkg, call, name + WHOLE)
    with pkg.LbmDem(LX, LY, r, x, y, strip=(128, 256), halo=12) as strip:
        for name, call in calls(strip):
            refused(pkg, call, name + WHOLE)
    with pkg.LbmDem(LX, LY, r, x, y, precision="f32") as sp:
        for name, call in calls(sp):
            refused(pkg, call, SP)
    assert os.listdir(tmp_path) == []


def test_checkpoints_do_not_carry_a_window(pkg, tmp_path):
    r, x, y = samples.to_metres(*samples.row_packing(LX, LY, 65, seed=29))
    with pkg.LbmDem(LX, LY, r, x, y) as a, pkg.LbmDem(LX, LY, r, x, y) as b:
        a.begin_mean(mu.ALL, 1)
        a.set_mean_output(mu.ALL, 3)
        a.renderScene(30); b.renderScene(30)
        assert a.mean_stats()["samples"] == len(range(0, 30, a.cfg.npDEM)) > 1
        a.checkpoint_save(str(tmp_path / "a.ckpt")); b.checkpoint_save(str(tmp_path / "b.ckpt"))
        assert (tmp_path / "a.ckpt").read_bytes() == (tmp_path / "b.ckpt").read_bytes()
        assert a.mean_stats()["present"] == 1   # (saving leaves the window alone)
    back = pkg.LbmDem.checkpoint_load(str(tmp_path / "a.ckpt"))
    try:
        assert back.mean_stats() == dict(present=0, mask=0, samples=0, hook_steps=0, bytes=0)
        back.renderScene(12)
        assert back.mean_stats()["samples"] == 0
        with pytest.raises(pkg.LbmDemError, match="no window is open"):
            back.mean_accumulators()
    finally:
        back.close()


def test_other_features_keep_theirs(pkg):
    """a vibrating handle with a probe-less lid, tracers and a scalar: the window samples what the restatement says"""
    r, x, y = g6()
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        sim.set_lid(0.01)
        sim.set_vibration(True)
        sim.set_tracers(np.array([[10.5, 20.25], [100.0, 150.0]]))
        sim.set_scalar(np.ones((LX, LY)), 0.8)
        sim.begin_mean(mu.ALL, 0)
        sim.renderScene(2 * sim.cfg.npDEM + 1)
        want = mu.window((LX, LY))
        mu.sample(want, mu.state(sim))
        sim.sample_mean()
        assert differing(sim.mean_accumulators(), want) == [] and sim.mean_stats()["samples"] == 1
        assert sim.tracer_stats()["hook_advances"] == 3 and sim.scalar_stats()["hook_steps"] == 3


def test_host_driver_writes_the_files(pkg, po, tmp_path):
    """`lbmdem <G6's sample> --steps 8000 --mean 4` in a process of its own: the two files of the run's one VTK event, byte for
    byte those of run_scene with set_mean_output(MEAN_ALL, 4). (The driver has the reference's frame cadence of 8000 sub-steps and
    no option for another: this is the shortest run of it that writes a frame.)"""
    z = np.load(os.path.join(REF_DIR, "inputs_and_table.npz"))
    sample = tmp_path / "g6.data"
    po.write_sample(str(sample), z["r_mm"], z["x_mm"], z["y_mm"])
    r, x, y = pkg.read_sample(str(sample))
    (tmp_path / "drv").mkdir(); (tmp_path / "py").mkdir()
    out = subprocess.run([EXE, str(sample), "--lx", str(LX), "--ly", str(LY), "--steps", "8000", "--mean", "4"], capture_output=True,
                         text=True, cwd=tmp_path / "drv", timeout=300)
    assert out.returncode == 0, out.stderr[-800:]
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        sim.set_mean_output(mu.ALL, 4)
        _, res = sim.run_scene(8000, str(tmp_path / "py"))
        assert res["nfile"] == 1
        fluid_steps = len(range(0, 8000, sim.cfg.npDEM))
    names = ["mean000000.vtk", "mean_profile000000.dat"]
    assert sorted(n for n in os.listdir(tmp_path / "drv") if n.startswith("mean")) == names
    for n in names:
        assert (tmp_path / "drv" / n).read_bytes() == (tmp_path / "py" / n).read_bytes(), n
    assert profile_samples(tmp_path / "py" / names[1]) == fluid_steps // 4 > 100
