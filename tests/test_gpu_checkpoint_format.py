"""GPU: the checkpoint format pinned to a file an earlier commit wrote, not to the code under test.

tests/golden/checkpoint_65x17.ckpt was written through checkpoint_save_async, with set_checkpoint_contents(CKPT_ALL), by the
library as it stood before the section table (CKPT_TABLE, lbmdem_internal.h) replaced the hand-written lists: the floor row of
test_gpu_async_checkpoint.py on 65 x 17 (5 grains; the row pitch is 32, not ly) 58 sub-steps into its run, with a pair list,
37 tracers (a section of 592 bytes), a dye field and a window of the velocity planes only, four fluid steps and one sample old;
it ends in the trailer "LBMCKSM2". That library reproduced the file byte for byte from a load -- checkpoint_save up to the
trailer, checkpoint_save_async all of it --, so every byte is compared here: the header, all fourteen sections, the extension
header and the trailer; no field is excluded."""
import os

import numpy as np
import pytest

from test_gpu_checkpoint_state import NAMES, TRAILER2, trailer2_of

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "checkpoint_65x17.ckpt")
LX, LY, N, NTR, PLANE = 65, 17, 5, 37, 65 * 32
CONTENTS = dict(mask=7, tracers=NTR, scalar_steps=4, mean_mask=1, mean_samples=1)


def first_difference(got, want, spans):
    if got == want:
        return None
    at = next((i for i, (u, v) in enumerate(zip(got, want)) if u != v), min(len(got), len(want)))
    return f"{len(got)} vs {len(want)} bytes, first difference at {at} {[n for n, (lo, hi) in spans.items() if lo <= at < hi]}"


def test_the_format_is_the_one_of_the_recorded_file(pkg, tmp_path):
    data = open(FIXTURE, "rb").read()
    body, spans = trailer2_of(data)                                # (every digest against numpy, every byte in one section)
    want = dict(header=464, r=8 * N, kin=72 * N, fhf=24 * N, gp=8 * N, offsets=4 * (N + 1), nbr=32, wallflags=N, obst=4 * PLANE,
                f=72 * PLANE, extras=120, tracers=16 * NTR, scalar_g=40 * PLANE, scalar_was=PLANE, mean_cnt=8 * PLANE,
                mean_S=16 * PLANE)
    assert {k: spans[k][1] - spans[k][0] for k in NAMES} == want
    assert len(data) == sum(want.values()) + TRAILER2 < 512 * 1024
    assert pkg.LbmDem.checkpoint_verify(FIXTURE) is True
    assert pkg.LbmDem.checkpoint_contents(FIXTURE) == CONTENTS
    sync, asyn = str(tmp_path / "sync.ckpt"), str(tmp_path / "async.ckpt")
    with pkg.LbmDem.checkpoint_load(FIXTURE) as sim:
        assert (sim.lx, sim.ly, sim.n, sim.nbsteps) == (LX, LY, N, 58)
        assert sim.tracer_stats()["tracers"] == NTR and sim.scalar_stats()["steps"] == 4 and sim.mean_stats()["samples"] == 1
        sim.set_checkpoint_contents(pkg.CKPT_ALL)                  # (the setting is not in the file)
        sim.checkpoint_save(sync)
        assert first_difference(open(sync, "rb").read(), body, spans) is None
        sim.set_async_checkpoint(1)
        sim.checkpoint_save_async(asyn)
        sim.output_drain()
        assert first_difference(open(asyn, "rb").read(), data, spans) is None
        sim.renderScene(3 * sim.cfg.npDEM)                         # three fluid steps: tracers, dye and window go on with it
        assert sim.nbsteps == 58 + 3 * sim.cfg.npDEM and np.isfinite(sim.f).all() and np.isfinite(sim.kinematics).all()
        assert sim.scalar_stats()["steps"] == 7 and sim.mean_stats()["samples"] == 2 and sim.tracer_stats()["advances"] == 7
