"""CPU: lbmdem_scene_schedule -- the events of the reference's main loop (main.c:1697-1777, 1880-1890) -- against a
step-by-step restatement of that loop: a plain loop over the step counter with one test per line of the reference. Host
arithmetic only, no device. All comparisons are exact."""
import numpy as np
import pytest

import golden_util as gu


def restated(cfg, nbsteps0, n, duration, fluid):
    """n x renderScene() + the loop's tail, one `if` per line of the reference"""
    ev = []
    npDEM, updateVerlet, stepFilm = cfg.npDEM, cfg.phys.updateVerlet, cfg.phys.stepFilm
    dt = np.float64(cfg.dt)
    nbsteps = nbsteps0
    nFile = nbsteps0 // stepFilm                                       # main.c:147
    for _ in range(n):
        if fluid and nbsteps % npDEM == 0:                             # main.c:1710 (inside #ifdef _FLUIDE_)
            if nbsteps % 400 == 0:                                     # main.c:1715
                ev.append(("CONSOLE_DENSITY", nbsteps, nFile))
        nbsteps += 1                                                   # main.c:1765
        if nbsteps % stepFilm == 0:                                    # main.c:1767
            ev.append(("VTK", nbsteps, nFile))
            nFile += 1                                                 # main.c:1771
        if nbsteps % 4000 == 0:                                        # main.c:1773
            ev.append(("DEM", nbsteps, nFile))
        if nbsteps % updateVerlet == 0:                                # main.c:1884
            ev.append(("STEPS_LINE", nbsteps, nFile))
        if duration >= 0 and np.float64(nbsteps) * dt > np.float64(duration):   # main.c:1890: while (nbsteps * dt <= duration)
            ev.append(("STOP", nbsteps, nFile))
            break
    return ev


def g4_cfg(pkg, **phys_changes):
    r, _, _ = gu.inputs_m("G4_coupled_256x200")
    phys = None
    if phys_changes:
        phys = pkg.derive(256, 200, r).phys
        for k, v in phys_changes.items():
            setattr(phys, k, v)
    return pkg.derive(256, 200, r, physics=phys)


def first_stop(cfg, lo, hi, duration):
    """the loop's predicate in numpy float64 on every s' of (lo, hi]"""
    s = np.arange(lo + 1, hi + 1, dtype=np.int64)
    over = s.astype(np.float64) * np.float64(cfg.dt) > np.float64(duration)
    return int(s[np.argmax(over)]) if over.any() else None


def test_g4_from_zero_for_16400_steps(pkg):
    cfg = g4_cfg(pkg)
    got = pkg.scene_schedule(cfg, 0, 16400)
    assert got == restated(cfg, 0, 16400, -1.0, True)
    kinds = [k for k, _, _ in got]
    assert kinds.count("VTK") == 2 and kinds.count("DEM") == 4 and kinds.count("STEPS_LINE") == 164 and "STOP" not in kinds
    lcm = np.lcm(cfg.npDEM, 400)
    assert kinds.count("CONSOLE_DENSITY") == (16400 - 1) // lcm + 1
    # write_DEM at 8000 uses the frame counter write_vtk has just advanced
    assert ("VTK", 8000, 0) in got and ("DEM", 8000, 1) in got and ("DEM", 4000, 0) in got


def test_start_in_mid_run(pkg):
    cfg = g4_cfg(pkg)
    for n in (0, 1, 22, 23, 24, 4223, 12100):
        assert pkg.scene_schedule(cfg, 3977, n) == restated(cfg, 3977, n, -1.0, True), n
    # the frame counter starts at nbsteps0 / stepFilm
    got = pkg.scene_schedule(cfg, 8001, 8000)
    assert got == restated(cfg, 8001, 8000, -1.0, True) and ("VTK", 16000, 1) in got


def test_without_the_fluid(pkg):
    cfg = g4_cfg(pkg)
    got = pkg.scene_schedule(cfg, 0, 16400, fluid=False)
    assert got == restated(cfg, 0, 16400, -1.0, False)
    assert all(k != "CONSOLE_DENSITY" for k, _, _ in got) and ("VTK", 8000, 0) in got


@pytest.mark.parametrize("updateVerlet,stepFilm", [(37, 900), (100, 1000), (250, 4000), (1, 3), (4000, 8000), (7, 7)])
def test_cadences_changed_through_phys(pkg, updateVerlet, stepFilm):
    cfg = g4_cfg(pkg, updateVerlet=updateVerlet, stepFilm=stepFilm)
    assert cfg.phys.updateVerlet == updateVerlet and cfg.phys.stepFilm == stepFilm
    for s0, n in ((0, 9000), (3977, 4223), (899, 2)):
        for fluid in (True, False):
            assert pkg.scene_schedule(cfg, s0, n, fluid=fluid) == restated(cfg, s0, n, -1.0, fluid), (s0, n, fluid)


def test_stop_on_a_plain_step_on_an_output_step_and_on_the_first(pkg):
    cfg = g4_cfg(pkg)
    dt = cfg.dt
    n = 16400
    # (a) a plain step: no other event on 5003
    # (b) the step of a VTK + DEM event: 8000
    # (c) s' = 1: any duration below dt, 0 included
    for want, durations in ((5003, [5002.5 * dt]), (8000, [7999.5 * dt]), (1, [0.0, 0.5 * dt])):
        for duration in durations:
            got = pkg.scene_schedule(cfg, 0, n, duration)
            assert first_stop(cfg, 0, n, duration) == want
            assert got[-1][:2] == ("STOP", want), got[-3:]
            assert got == restated(cfg, 0, n, duration, True)
    got = pkg.scene_schedule(cfg, 0, n, 7999.5 * dt)
    assert got[-4:] == [("VTK", 8000, 0), ("DEM", 8000, 1), ("STEPS_LINE", 8000, 1), ("STOP", 8000, 1)]
    assert [e for e in pkg.scene_schedule(cfg, 0, n, 5002.5 * dt) if e[1] == 5003] == [("STOP", 5003, 0)]


def test_stop_is_the_loops_own_predicate_at_the_rounding_edge(pkg):
    """durations that ARE a product s * dt, and their float64 neighbours: the stop is the first s' for which the product
    compares greater, whatever a division would say"""
    cfg = g4_cfg(pkg)
    dt = np.float64(cfg.dt)
    for s in (1, 2, 3, 7, 399, 400, 4000, 5003, 8000, 12345, 16399):
        prod = np.float64(s) * dt
        for duration in (float(prod), float(np.nextafter(prod, 0.0)), float(np.nextafter(prod, np.inf))):
            want = first_stop(cfg, 0, 16400, duration)
            got = pkg.scene_schedule(cfg, 0, 16400, duration)
            assert got[-1][:2] == ("STOP", want), (s, duration)
            assert got == restated(cfg, 0, 16400, duration, True), (s, duration)
    # a start beyond the stop: the do-while still makes one sub-step
    got = pkg.scene_schedule(cfg, 3977, 500, 10.5 * float(dt))
    assert got == [("STOP", 3978, 0)] == restated(cfg, 3977, 500, 10.5 * float(dt), True)
    # a stop beyond the range: none listed
    got = pkg.scene_schedule(cfg, 0, 5000, 5000.5 * float(dt))
    assert all(k != "STOP" for k, _, _ in got) and got == restated(cfg, 0, 5000, 5000.5 * float(dt), True)


def test_bad_arguments_are_refused(pkg):
    cfg = g4_cfg(pkg)
    for args in ((-1, 10), (0, -1)):
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.scene_schedule(cfg, *args)
        assert e.value.code == -1
    bad = g4_cfg(pkg)
    bad.phys.stepFilm = 0
    with pytest.raises(pkg.LbmDemError):
        pkg.scene_schedule(bad, 0, 10)


def test_sizing_call_and_short_buffers(pkg):
    import ctypes as C
    cfg = g4_cfg(pkg)
    L = pkg.load_library()
    count = C.c_long(-1)
    assert L.lbmdem_scene_schedule(C.byref(cfg), 0, 16400, -1.0, 1, None, 0, C.byref(count)) == 0
    full = pkg.scene_schedule(cfg, 0, 16400)
    assert count.value == len(full)
    ev = (pkg.SceneEvent * 4)()
    assert L.lbmdem_scene_schedule(C.byref(cfg), 0, 16400, -1.0, 1, ev, 3, C.byref(count)) == 0
    assert count.value == len(full)
    assert [(pkg.SCENE_KINDS[e.kind], e.step, e.nfile) for e in ev[:3]] == full[:3] and ev[3].step == 0 and ev[3].kind == 0
