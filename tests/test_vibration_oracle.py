"""CPU: the checker of the vibrating walls (the reference's vib = 1, main.c:1700-1705) and the library's host-side wall
schedule (lbmdem_vibration_schedule) against it. No GPU."""
import numpy as np
import pytest

import golden_util as gu
import vib_util as vu


def test_wrapper_with_zero_amplitude_is_the_oracle(pkg, po):
    """amp = 0: the clock runs, the walls stay -- 300 sub-steps equal ora_steps bit for bit"""
    r, x1, x2 = gu.inputs_m("G4_coupled_256x200")
    ora = po.Oracle(256, 200, r, x1, x2)
    vib = vu.VibOracle(256, 200, r, x1, x2, phys=vu.physics(pkg, freq=5.0, amp=0.0, dtt=0.0))
    ora.steps(300)
    vib.vib_steps(300)
    assert np.array_equal(vib.get_f(), ora.get_f())
    assert np.array_equal(vib.get_obst(), ora.get_obst())
    assert np.array_equal(vib.get_fhf(), ora.get_fhf())
    assert np.array_equal(vib.get_grains(), ora.get_grains())
    assert vib.walls()["t"] > 0.0


def test_wrapper_wall_trajectory_is_the_restated_reference(pkg):
    """with vibration: t, Mgx, Mdx after every sub-step equal main.c:1700-1705 + 1555-1561 restated in Python floats"""
    r, x1, x2 = gu.inputs_m("G4_coupled_256x200")
    phys = vu.physics(pkg, freq=4000.0, amp=5e-6)
    cfg = pkg.derive(256, 200, r, physics=phys)
    phys.dtt = 150 * cfg.dt
    cfg.phys.dtt = phys.dtt
    vib = vu.VibOracle(256, 200, r, x1, x2, phys=phys)
    want = vu.restated_walls(cfg, 0, 260)
    for k in range(260):
        vib.vib_steps(1)
        w = vib.walls()
        assert (w["t"], w["Mgx"], w["Mdx"]) == tuple(want[k, :3]), k
    assert want[-1, 1] - cfg.Mgx > cfg.dx              # the side wall has moved by more than a node


@pytest.mark.parametrize("dry", [False, True])
def test_library_schedule_equals_the_wrapper(pkg, dry):
    """lbmdem_vibration_schedule: the walls of every sub-step across four Verlet rebuilds (Mdx reset, main.c:1555-1561)
    and across dtt (the reset switches to 1e-3 * lx at sub-step 200), started mid-run from the wrapper's own state"""
    r, x1, x2 = gu.inputs_m("G4_coupled_256x200")
    phys = vu.physics(pkg, freq=3000.0, amp=2e-6)
    cfg = pkg.derive(256, 200, r, physics=phys)
    phys.dtt = 150.5 * cfg.dt
    cfg.phys.dtt = phys.dtt
    vib = vu.VibOracle(256, 200, r, x1, x2, phys=phys)
    step = vib.vib_steps_dry if dry else vib.vib_steps
    got = pkg.vibration_schedule(cfg, 0, 420)
    start = None
    for k in range(420):
        if k == 37:   # a schedule that starts mid-run from the walls as they are
            w = vib.walls()
            c2 = pkg.Config.from_buffer_copy(cfg)
            c2.phys.t, c2.Mgx, c2.Mdx = w["t"], w["Mgx"], w["Mdx"]
            start = pkg.vibration_schedule(c2, 37, 420 - 37)
        step(1)
        w = vib.walls()
        row = (w["t"], w["Mgx"], w["Mdx"])
        assert tuple(got[k, :3]) == row, k
        if start is not None:
            assert tuple(start[k - 37, :3]) == row, k
    want = vu.restated_walls(cfg, 0, 420)
    assert np.array_equal(got, want)                     # incl. the top wall's amp*freq*cos(freq*t)
    assert got[100, 2] == 1e-3 * 256 / 10                # reset before dtt ...
    assert got[200, 2] == 1e-3 * 256                     # ... and past it
    assert got[199, 2] != got[100, 2] and got[199, 1] != got[100, 1]   # between the resets both walls move


def test_schedule_rejects_bad_arguments(pkg):
    r, _, _ = gu.inputs_m("G4_coupled_256x200")
    cfg = pkg.derive(256, 200, r)
    with pytest.raises(pkg.LbmDemError):
        pkg.vibration_schedule(cfg, -1, 3)
