"""GPU: checkpoints that carry the tracers, the passive scalar and the averaging window (lbmdem_set_checkpoint_contents,
lbmdem_checkpoint_contents; include/lbmdem_hip.h) -- the round trip through the synchronous and the background writer, subsets,
slots that grow, an interrupted lbmdem_run_scene, the host driver, the refusals. Every comparison is exact: a run continued from a
file holds the same bits as the uninterrupted one.

The lattice and the packing are those of the three tests that pin the default (test_checkpoints_do_not_carry_*): npDEM is 12
there, so the fluid steps are the sub-steps 0, 12, 24, ... A state is set up after 6 sub-steps; 30 more make two fluid steps, so
that a window with every = 3 is saved out of phase (hook_steps % 3 == 2), without a sample so far; the case `54` runs on to four
fluid steps, which puts a sample into the file as well (hook_steps % 3 == 1)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import samples
from test_checkpoint_digest import digest_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
LX, LY = 256, 200
PLANE = LX * ((LY + 15) // 16 * 16)
TAU = 0.8
NAMES = ("header", "r", "kin", "fhf", "gp", "offsets", "nbr", "wallflags", "obst", "f",
         "extras", "tracers", "scalar_g", "scalar_was", "mean_cnt", "mean_S")
TRAILER2 = 16 + 24 * len(NAMES)
MEAN_U, MEAN_ALL = 1, 31


def packing():
    return samples.to_metres(*samples.row_packing(LX, LY, 65, seed=29))


def seeds(n):
    return np.random.default_rng(n).uniform((0.5, 0.5), (LX - 1.5, LY - 1.5), (n, 2))


def dressed(pkg, ntracers=63, mean_mask=MEAN_ALL, physics=None):
    """a handle six sub-steps into its run with tracers, a random scalar and a window that samples every third fluid step"""
    r, x, y = packing()
    sim = pkg.LbmDem(LX, LY, r, x, y, physics=physics)
    sim.renderScene(6)
    sim.set_tracers(seeds(ntracers))
    sim.set_scalar(np.random.default_rng(67).normal(1.0, 0.5, (LX, LY)), TAU)
    sim.begin_mean(mean_mask, 3)
    return sim


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def everything(sim):
    """all a continuation can differ in, as arrays and dicts that compare with =="""
    g, was = sim.scalar_state()
    out = dict(tracers=sim.tracers, scalar_g=g, scalar_was=was, f=sim.f, obst=sim.obst, kin=sim.kinematics, fhf=sim.fhf,
               gp=sim.grain_pressure)
    out.update({"mean_" + k: v for k, v in sim.mean_accumulators().items()})
    return out, dict(nbsteps=sim.nbsteps, tracers=sim.tracer_stats(), scalar=sim.scalar_stats(), mean=sim.mean_stats())


def assert_same(a, b):
    (xa, ca), (xb, cb) = everything(a), everything(b)
    assert ca == cb
    assert xa.keys() == xb.keys()
    for k in xa:
        assert xa[k].shape == xb[k].shape and np.array_equal(bits(xa[k]), bits(xb[k])), k


def trailer2_of(data):
    """-> (the bytes in front of the trailer "LBMCKSM2", {name: (first, end) in them}); every digest checked against numpy"""
    assert data[-TRAILER2:-TRAILER2 + 8] == b"LBMCKSM2", data[-TRAILER2:-TRAILER2 + 8]
    assert struct.unpack("<ii", data[-TRAILER2 + 8:-TRAILER2 + 16]) == (len(NAMES), 0)
    ent = np.frombuffer(data[-TRAILER2 + 16:], "<u8").reshape(len(NAMES), 3)
    body, at, spans = data[:-TRAILER2], 0, {}
    for name, (nb, s1, s2) in zip(NAMES, ent):
        spans[name] = (at, at + int(nb))
        assert (int(s1), int(s2)) == (digest_numpy(body[at:at + int(nb)]) if nb else (0, 0)), name
        at += int(nb)
    assert at == len(body)
    return body, spans


# ---- 1. the round trip, bit for bit ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["all", "velocity_window", "one_tracer", "54"])
def test_a_restart_continues_bit_equal(pkg, tmp_path, case):
    ntr = 1 if case == "one_tracer" else 63
    mask = MEAN_U if case == "velocity_window" else MEAN_ALL
    before = 54 if case == "54" else 30
    ck = str(tmp_path / "state.ckpt")
    with dressed(pkg, ntr, mask) as a:
        a.set_checkpoint_contents(pkg.CKPT_ALL)
        a.renderScene(before)
        st = a.mean_stats()
        assert st["hook_steps"] % 3 != 0 and st["samples"] == (1 if case == "54" else 0), st
        a.checkpoint_save(ck)
        assert pkg.LbmDem.checkpoint_verify(ck) is False         # (the synchronous file has no trailer, as ever)
        assert pkg.LbmDem.checkpoint_contents(ck) == dict(mask=7, tracers=ntr, scalar_steps=a.scalar_stats()["steps"],
                                                          mean_mask=mask, mean_samples=st["samples"])
        nsel = len(a.mean_accumulators()) - 2
        plain = 120 + 16 * ntr + 41 * PLANE + 8 * PLANE + 8 * nsel * PLANE
        with pkg.LbmDem.checkpoint_load(ck) as b:
            assert_same(a, b)                                     # as loaded
            b.checkpoint_save(str(tmp_path / "plain.ckpt"))       # (the setting is not in the file: b saves the plain file)
            assert os.path.getsize(ck) - os.path.getsize(tmp_path / "plain.ckpt") == plain
            a.renderScene(36); b.renderScene(36)
            assert a.mean_stats()["samples"] > st["samples"]
            assert_same(a, b)
            a.advance_tracers(); a.step_scalar(); a.sample_mean()  # by hand, too
            b.advance_tracers(); b.step_scalar(); b.sample_mean()
            assert_same(a, b)


# ---- 2. subsets -------------------------------------------------------------------------------------------------------------------

def test_only_what_is_selected_and_present(pkg, tmp_path):
    ck, other = str(tmp_path / "tracers.ckpt"), str(tmp_path / "none.ckpt")
    with dressed(pkg) as a:
        a.renderScene(30)
        a.set_checkpoint_contents(pkg.CKPT_TRACERS)
        a.checkpoint_save(ck)
        assert pkg.LbmDem.checkpoint_contents(ck) == dict(mask=1, tracers=63, scalar_steps=0, mean_mask=0, mean_samples=0)
        with pkg.LbmDem.checkpoint_load(ck) as b:
            assert b.tracer_stats() == a.tracer_stats() and np.array_equal(bits(a.tracers), bits(b.tracers))
            assert b.scalar_stats() == dict(present=0, steps=0, hook_steps=0)
            assert b.mean_stats() == dict(present=0, mask=0, samples=0, hook_steps=0, bytes=0)
        a.set_checkpoint_contents(0)
        a.checkpoint_save(other)                                  # off again: today's file
        a.set_scalar(None)
        a.set_checkpoint_contents(pkg.CKPT_SCALAR)                # asked for, not there: the same file, byte for byte
        a.checkpoint_save(ck)
        assert open(ck, "rb").read() == open(other, "rb").read()
        assert pkg.LbmDem.checkpoint_contents(ck)["mask"] == 0
        a.set_async_checkpoint(1)
        a.checkpoint_save_async(ck); a.output_drain()
        data = open(ck, "rb").read()
        assert data[:-256] == open(other, "rb").read() and data[-256:-248] == b"LBMCKSM1"   # ... and the trailer of ten sections


# ---- 3. the background path ------------------------------------------------------------------------------------------------------

def test_the_async_file_is_the_synchronous_one_with_a_trailer(pkg, tmp_path):
    sync, asyn, bad = (str(tmp_path / n) for n in ("sync.ckpt", "async.ckpt", "bad.ckpt"))
    with dressed(pkg) as a:
        a.set_checkpoint_contents(pkg.CKPT_ALL)
        a.set_async_checkpoint(1)
        a.renderScene(54)
        a.checkpoint_save(sync)
        a.checkpoint_save_async(asyn)
        a.renderScene(36)                                          # the run goes on at once: nothing of it reaches the file
        a.output_drain()
        data = open(asyn, "rb").read()
        body, spans = trailer2_of(data)
        assert body == open(sync, "rb").read()
        want = dict(extras=120, tracers=16 * 63, scalar_g=40 * PLANE, scalar_was=PLANE, mean_cnt=8 * PLANE, mean_S=88 * PLANE)
        assert {k: spans[k][1] - spans[k][0] for k in want} == want
        assert pkg.LbmDem.checkpoint_verify(asyn) is True
        lo, hi = spans["mean_S"]
        for where, name in ((lo + (hi - lo) // 3, "mean_S"), (spans["scalar_was"][0] + 77, "scalar_was"), (spans["tracers"][1] - 1, "tracers")):
            torn = bytearray(data)
            torn[where] ^= 0x04
            open(bad, "wb").write(bytes(torn))
            with pytest.raises(pkg.LbmDemError, match=f"section '{name}'"):
                pkg.LbmDem.checkpoint_load(bad)
        with pkg.LbmDem.checkpoint_load(asyn) as b:
            b.renderScene(36)
            assert_same(a, b)
        assert a.output_stats_checkpoint()["failed"] == 0


def test_the_loader_trusts_nothing_of_a_file_without_digests(pkg, tmp_path):
    """the synchronous file has no trailer to catch these: the loader's own checks do"""
    ck, bad = str(tmp_path / "good.ckpt"), str(tmp_path / "bad.ckpt")
    with dressed(pkg) as a:
        a.set_checkpoint_contents(pkg.CKPT_ALL)
        a.renderScene(30)
        a.checkpoint_save(ck)
    data = open(ck, "rb").read()
    ext = len(data) - (120 + 16 * 63 + 41 * PLANE + 8 * PLANE + 88 * PLANE)
    assert data[ext:ext + 8] == b"LBMXTRA1"
    nan = struct.pack("<d", float("nan"))
    edits = {"tracer outside": (ext + 120 + 16 * 5, struct.pack("<d", LX - 0.5)), "tracer NaN": (ext + 120 + 16 * 7 + 8, nan),
             "tau": (ext + 56, struct.pack("<d", 0.25)), "tau NaN": (ext + 56, nan), "count": (ext + 24, struct.pack("<q", 1 << 40)),
             "was": (ext + 120 + 16 * 63 + 40 * PLANE + 1000, b"\2"), "mean mask": (ext + 88, struct.pack("<i", 32)),
             "nsel": (ext + 96, struct.pack("<i", 2)), "samples": (ext + 104, struct.pack("<q", -3)), "mask": (ext + 8, struct.pack("<i", 9)),
             "plane": (ext + 16, struct.pack("<q", PLANE - 16))}
    for what, (at, new) in edits.items():
        torn = bytearray(data)
        torn[at:at + len(new)] = new
        open(bad, "wb").write(bytes(torn))
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.LbmDem.checkpoint_load(bad)
        assert e.value.code == -1, (what, str(e.value))
    for keep in (ext + 60, ext + 120 + 100, len(data) - 1):       # cut inside the extension
        open(bad, "wb").write(data[:keep])
        with pytest.raises(pkg.LbmDemError, match="extension"):
            pkg.LbmDem.checkpoint_load(bad)
    open(bad, "wb").write(data[:ext])                              # cut in front of it: a plain file
    with pkg.LbmDem.checkpoint_load(bad) as b:
        assert b.tracer_stats()["tracers"] == 0 and b.scalar_stats()["present"] == 0 and b.mean_stats()["present"] == 0


# ---- 4. slots that grow -----------------------------------------------------------------------------------------------------------

def test_slots_grow_with_the_state(pkg, tmp_path):
    one, two = str(tmp_path / "one.ckpt"), str(tmp_path / "two.ckpt")
    r, x, y = packing()
    with pkg.LbmDem(LX, LY, r, x, y) as a:
        a.set_checkpoint_contents(pkg.CKPT_ALL)
        a.set_async_checkpoint(1)                                  # sized for the plain file
        a.renderScene(6)
        a.set_scalar(np.random.default_rng(67).normal(1.0, 0.5, (LX, LY)), TAU)
        a.begin_mean(MEAN_ALL, 1)
        a.renderScene(30)
        a.checkpoint_save_async(one)
        a.set_scalar(None)
        a.renderScene(12)
        a.checkpoint_save_async(two)
        a.output_drain()
        st = a.output_stats_checkpoint()
        assert (st["queued"], st["written"], st["failed"]) == (2, 2, 0), st
        assert pkg.LbmDem.checkpoint_verify(one) is True and pkg.LbmDem.checkpoint_verify(two) is True
        c1, c2 = pkg.LbmDem.checkpoint_contents(one), pkg.LbmDem.checkpoint_contents(two)
        assert c1["mask"] == pkg.CKPT_SCALAR | pkg.CKPT_MEAN and c1["scalar_steps"] == 2 and c1["mean_samples"] == 2
        assert c2["mask"] == pkg.CKPT_MEAN and c2["scalar_steps"] == 0 and c2["mean_samples"] == 3
        assert os.path.getsize(one) - os.path.getsize(two) == 41 * PLANE
        trailer2_of(open(one, "rb").read()); trailer2_of(open(two, "rb").read())
        with pkg.LbmDem.checkpoint_load(two) as b:
            assert_same_window(a, b)


def assert_same_window(a, b):
    assert a.mean_stats() == b.mean_stats()
    wa, wb = a.mean_accumulators(), b.mean_accumulators()
    for k in wa:
        assert np.array_equal(bits(wa[k]), bits(wb[k])), k


# ---- 5. an interrupted lbmdem_run_scene --------------------------------------------------------------------------------------------

FILM, EVERY, STEPS, STOP = 60, 90, 200, 100      # frames behind the sub-steps 60, 120, 180; the checkpoint of 90 lies between two
LATE = re.compile(r"(tracers|scalar|mean|mean_profile)\d{6}\.(vtk|dat)")


def scene_sim(pkg):
    r, x, y = packing()
    phys = pkg.derive(LX, LY, r).phys
    phys.stepFilm = FILM
    sim = dressed(pkg, physics=phys)
    outputs_on(sim)
    return sim


def outputs_on(sim):
    sim.set_tracer_output(True)
    sim.set_scalar_output(True)
    sim.set_mean_output(MEAN_ALL, 3)


@pytest.mark.parametrize("mode", ["synchronous", "slots"])
def test_an_interrupted_scene_writes_the_same_files(pkg, tmp_path, mode):
    da, db, dc = (tmp_path / n for n in "abc")
    for d in (da, db, dc):
        d.mkdir()
    ck = str(tmp_path / "run.ckpt")
    with scene_sim(pkg) as a:
        a.run_scene(STEPS - 6, outdir=str(da))
        final = everything(a)
    with scene_sim(pkg) as b:
        b.set_checkpoint_contents(pkg.CKPT_ALL)
        if mode == "slots":
            b.set_async_checkpoint(1)
        b.set_checkpoint_every(EVERY, ck)
        b.run_scene(STOP - 6, outdir=str(db))                      # stopped behind the checkpoint of 90, in front of the frame of 120
    assert pkg.LbmDem.checkpoint_verify(ck) is (mode == "slots")
    got = pkg.LbmDem.checkpoint_contents(ck)
    assert got["mask"] == 7 and got["tracers"] == 63 and got["mean_mask"] == MEAN_ALL, got
    with pkg.LbmDem.checkpoint_load(ck) as c:
        assert c.nbsteps == EVERY and c.mean_stats()["hook_steps"] % 3 != 0
        outputs_on(c)                                              # (the output settings are not in the file)
        c.run_scene(STEPS - EVERY, outdir=str(dc))
        now = everything(c)
    assert now[1] == final[1]
    for k in final[0]:
        assert np.array_equal(bits(final[0][k]), bits(now[0][k])), k
    late = sorted(p.name for p in dc.iterdir() if LATE.fullmatch(p.name))
    want = sorted(f % k for k in (1, 2) for f in ("tracers%.6i.vtk", "scalar%.6i.vtk", "mean%.6i.vtk", "mean_profile%.6i.dat"))
    assert late == want, late
    for n in late:
        assert (da / n).read_bytes() == (dc / n).read_bytes(), n


def test_a_scene_opens_a_new_window_where_the_loaded_one_is_another(pkg, tmp_path):
    """the one-shot mark: only a window of the output setting's mask and cadence goes on, and only once"""
    ck = str(tmp_path / "w.ckpt")
    with dressed(pkg) as a:
        a.set_checkpoint_contents(pkg.CKPT_MEAN)
        a.renderScene(54)
        assert a.mean_stats()["samples"] == 1
        a.checkpoint_save(ck)
    for mask, every, goes_on in ((MEAN_ALL, 3, True), (MEAN_ALL, 2, False), (MEAN_U, 3, False)):
        with pkg.LbmDem.checkpoint_load(ck) as b:
            b.set_mean_output(mask, every)
            b.run_scene(0, outdir=str(tmp_path))
            assert b.mean_stats()["samples"] == (1 if goes_on else 0), (mask, every)
            b.run_scene(0, outdir=str(tmp_path))                   # the second call begins afresh, as it always has
            assert b.mean_stats()["samples"] == 0


# ---- 6. the host driver ------------------------------------------------------------------------------------------------------------

def test_host_driver_restarts_with_its_state(pkg, po, tmp_path):
    """frames come every 8000 sub-steps in the driver: 8100 straight through against 5000, a restart, and on to 8100"""
    r, x, y = samples.row_packing(LX, LY, 65, seed=29)
    flags = ["--tracers", "4x4", "--dye", "40,40,120,120", "--dye-tau", "0.8", "--mean", "2", "--checkpoint", "run.ckpt",
             "--checkpoint-state"]

    def drive(d, args):
        d.mkdir(exist_ok=True)
        sample = d / "packing.data"
        if not sample.exists():
            po.write_sample(str(sample), r, x, y)
        out = subprocess.run([EXE, str(sample), "--lx", str(LX), "--ly", str(LY)] + flags + args, capture_output=True, text=True,
                             cwd=d, timeout=600)
        assert out.returncode == 0, (out.stdout[-400:], out.stderr[-1200:])
        return out

    whole = drive(tmp_path / "whole", ["--steps", "8100"])
    assert "Restored with it" not in whole.stdout
    drive(tmp_path / "cut", ["--steps", "5000"])
    assert not list((tmp_path / "cut").glob("tracers*.vtk"))
    got = pkg.LbmDem.checkpoint_contents(str(tmp_path / "cut" / "run.ckpt"))
    assert got["mask"] == 7 and got["tracers"] == 16 and got["mean_mask"] == MEAN_ALL and got["scalar_steps"] == 417, got
    tail = drive(tmp_path / "cut", ["--restart", "run.ckpt", "--steps", "8100"])
    assert "Restarted from run.ckpt at step 5000" in tail.stdout
    line = [l for l in tail.stdout.splitlines() if l.startswith("Restored with it:")]
    assert len(line) == 1 and "16 tracers" in line[0] and "the dye" in line[0] and "averaging window" in line[0], tail.stdout[-600:]
    fd = lambda o: re.search(r"^final_density: ([0-9.]+)$", o.stderr, re.M).group(1)
    assert fd(tail) == fd(whole)
    names = ["tracers000000.vtk", "scalar000000.vtk", "mean000000.vtk", "mean_profile000000.dat", "scalar.data", "DEM000001.dat"]
    for n in names:
        assert (tmp_path / "whole" / n).read_bytes() == (tmp_path / "cut" / n).read_bytes(), n
    assert (tmp_path / "whole" / "run.ckpt").read_bytes() == (tmp_path / "cut" / "run.ckpt").read_bytes()
    # without --checkpoint-state the file is the plain one and a restart seeds afresh
    flags.remove("--checkpoint-state")
    drive(tmp_path / "plain", ["--steps", "24"])
    again = drive(tmp_path / "plain", ["--restart", "run.ckpt", "--steps", "48"])
    assert "Restarted from" in again.stdout and "Restored with it" not in again.stdout


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(pkg, tmp_path):
    r, x, y = packing()
    with pkg.LbmDem(LX, LY, r, x, y) as sim:
        for mask in (8, -1, 15):
            with pytest.raises(pkg.LbmDemError, match="bad mask") as e:
                sim.set_checkpoint_contents(mask)
            assert e.value.code == -1
        sim.set_checkpoint_contents(pkg.CKPT_ALL)
        sim.set_checkpoint_contents(0)
    with pkg.LbmDem(LX, LY, r, x, y, strip=(0, 128), halo=2) as strip:
        with pytest.raises(pkg.LbmDemError, match="needs the whole lattice and all grains on this handle") as e:
            strip.set_checkpoint_contents(pkg.CKPT_TRACERS)
        assert e.value.code == -1
        strip.set_checkpoint_contents(0)                           # off is what a strip has anyway
    with pkg.LbmDem(LX, LY, r, x, y) as dist:
        dist.dist_enable()
        with pytest.raises(pkg.LbmDemError, match="needs the whole lattice and all grains on this handle"):
            dist.set_checkpoint_contents(pkg.CKPT_ALL)
    if os.path.exists(pkg.SP_LIB_PATH):                            # the float build has no checkpoints at all
        with pkg.LbmDem(LX, LY, r, x, y, precision="f32") as sp:
            with pytest.raises(pkg.LbmDemError, match="single-precision") as e:
                sp.set_checkpoint_contents(pkg.CKPT_ALL)
            assert e.value.code == -1
    assert list(tmp_path.iterdir()) == []
