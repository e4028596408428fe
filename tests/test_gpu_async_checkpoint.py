"""GPU: checkpoints written in the background (lbmdem_set_async_checkpoint / lbmdem_checkpoint_save_async), on a cadence
(lbmdem_set_checkpoint_every), replaced atomically, with digests (lbmdem_checkpoint_verify) -- the snapshot kernel against the
synchronous save, a snapshot although the run goes on at once, corruption, the cadence inside lbmdem_run_scene, back-pressure with
one slot, the writer's errors, the refusals, a replayed run, and the host driver. All comparisons are exact.

Unless a case says otherwise files are compared like this: the file of lbmdem_checkpoint_save at the same state equals the async
file's bytes in front of its trailer, and the trailer equals the numpy digest of those bytes, section by section."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
from test_checkpoint_digest import digest_numpy
from test_gpu_run_scene import without_clock
from test_gpu_vibration import _inputs as _vib_inputs, _shaker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "2d-lbm-dem_amd", "host", "lbmdem")
SECTIONS = ("header", "r", "kin", "fhf", "gp", "offsets", "nbr", "wallflags", "obst", "f")
TRAILER = 16 + 24 * len(SECTIONS)
FIELDS = ("grain_pressure", "grain_velocity", "grain_acceleration", "fluid_pressure", "fluid_velocity")


def g4():
    return (256, 200) + tuple(gu.inputs_m("G4_coupled_256x200"))


def floor_row(lx, ly):
    """a row of grains of 0.5 mm on the floor (a node is 0.1 mm), some in contact, as test_gpu_async_output.py builds it"""
    x1 = np.arange(1.0e-3, lx * 1e-4 - 1.0e-3, 1.02e-3)
    return lx, ly, np.full(len(x1), 0.5e-3), x1, np.full(len(x1), 0.75e-3)


def trailer_of(data):
    """-> (the bytes in front of the trailer, [(bytes, S1, S2)] per section)"""
    assert len(data) > TRAILER and data[-TRAILER:-TRAILER + 8] == b"LBMCKSM1", data[-TRAILER:-TRAILER + 8]
    assert struct.unpack("<ii", data[-TRAILER + 8:-TRAILER + 16]) == (len(SECTIONS), 0)
    ent = np.frombuffer(data[-TRAILER + 16:], "<u8").reshape(len(SECTIONS), 3)
    return data[:-TRAILER], [tuple(int(v) for v in row) for row in ent]


def section_spans(entries):
    at, out = 0, {}
    for name, (nb, _, _) in zip(SECTIONS, entries):
        out[name] = (at, at + nb)
        at += nb
    return out


def check_async_file(async_path, sync_path, sim=None):
    a, s = open(async_path, "rb").read(), open(sync_path, "rb").read()
    body, ent = trailer_of(a)
    if body != s:
        bad = next((i for i, (u, v) in enumerate(zip(body, s)) if u != v), None)
        where = [n for n, (lo, hi) in section_spans(ent).items() if bad is not None and lo <= bad < hi]
        raise AssertionError(f"{len(body)} vs {len(s)} bytes, first difference at {bad} {where}")
    spans = section_spans(ent)
    assert spans["f"][1] == len(body)                     # every byte in front of the trailer belongs to exactly one section
    for name, (nb, s1, s2) in zip(SECTIONS, ent):
        lo, hi = spans[name]
        assert digest_numpy(body[lo:hi]) == (s1, s2), name
    if sim is not None:
        n, plane = sim.n, sim.lx * ((sim.ly + 15) // 16 * 16)
        want = dict(r=8 * n, kin=72 * n, fhf=24 * n, gp=8 * n, offsets=4 * (n + 1), wallflags=n, obst=4 * plane, f=72 * plane)
        for name, nb in want.items():
            assert spans[name][1] - spans[name][0] == nb, name
    return spans


def same_restart(a, b):
    """the comparison of test_gpu_parity.py::test_checkpoint_restart_is_bit_identical"""
    assert a.nbsteps == b.nbsteps
    assert np.isfinite(a.kinematics).all()
    assert np.array_equal(a.f, b.f)
    assert np.array_equal(a.obst, b.obst)
    assert np.array_equal(a.kinematics, b.kinematics)
    assert np.array_equal(a.fhf, b.fhf)
    assert np.array_equal(a.grain_pressure, b.grain_pressure)


def no_tmp_files(d):
    left = [str(p) for p in d.rglob("*.tmp")]
    assert left == [], left


# ---- 1. the kernel alone, against the synchronous save ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["G4", "83x37", "65x17"])
def test_async_file_equals_the_synchronous_save(pkg, tmp_path, case):
    """before the first step (no pair list: zero offsets, no entries), after 60 sub-steps, and at a counter that is neither a
    fluid step nor a rebuild. The floor rows have 7 and 5 grains on lattices whose row pitch is not ly: n is no multiple of 8,
    wallflags (n bytes) and offsets (4 (n + 1) bytes) end inside a 16-byte chunk, the grains' arrays start 8 (mod 16) bytes in."""
    lx, ly, r, x1, x2 = g4() if case == "G4" else floor_row(*(int(v) for v in case.split("x")))
    if case != "G4":
        assert len(r) % 8 != 0 and len(r) % 2 == 1 and ly % 16 != 0
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_async_checkpoint(1)
    npdem, verlet = sim.cfg.npDEM, sim.cfg.phys.updateVerlet
    odd = next((k for k in range(1, 50) if (60 + k) % npdem != 0 and (60 + k) % verlet != 0), 1)
    for tag, steps in (("start", 0), ("s60", 60), ("odd", odd)):
        sim.renderScene(steps)
        A, B = str(tmp_path / (tag + ".sync")), str(tmp_path / (tag + ".async"))
        sim.checkpoint_save_async(B)
        sim.checkpoint_save(A)
        sim.output_drain()
        spans = check_async_file(B, A, sim)
        nbr = spans["nbr"][1] - spans["nbr"][0]
        assert (nbr == 0) == (tag == "start") and nbr % 8 == 0      # the list is symmetric: every pair twice
        print(f"{case} {tag}: n {sim.n} step {sim.nbsteps} nbr entries {nbr // 4} file {os.path.getsize(B)} bytes")
        assert pkg.LbmDem.checkpoint_verify(B) is True and pkg.LbmDem.checkpoint_verify(A) is False
    assert sim.nbsteps == 60 + odd
    st = sim.output_stats_checkpoint()
    assert (st["queued"], st["written"], st["failed"]) == (3, 3, 0)
    no_tmp_files(tmp_path)
    sim.close()


def test_a_pair_list_with_an_odd_number_of_pairs(pkg, tmp_path):
    """the nbr section is 8 bytes per pair: with an odd number of pairs it ends half way through a 16-byte chunk. Rows of
    2 .. 6 touching grains on 83 x 37: neighbouring grains pair up, so both parities occur."""
    tails = {}
    for n in range(2, 7):
        lx, ly, r, x1, x2 = floor_row(83, 37)
        sim = pkg.LbmDem(lx, ly, r[:n], x1[:n], x2[:n])
        sim.set_async_checkpoint(1)
        sim.renderScene(25)
        A, B = str(tmp_path / f"{n}.sync"), str(tmp_path / f"{n}.async")
        sim.checkpoint_save_async(B)
        sim.checkpoint_save(A)
        sim.output_drain()
        spans = check_async_file(B, A, sim)
        tails[n] = (spans["nbr"][1] - spans["nbr"][0]) % 16
        sim.close()
    print("nbr bytes mod 16 by grain count:", tails)
    assert set(tails.values()) == {0, 8}, tails


# ---- 2. a snapshot although the run goes on ----------------------------------------------------------------------------------------

def test_a_checkpoint_holds_the_state_it_was_asked_at(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_async_checkpoint(2)
    n1 = 2 * sim.cfg.npDEM + 5
    sim.renderScene(n1)
    A, B = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    sim.checkpoint_save(A)
    sim.checkpoint_save_async(B)
    sim.renderScene(60)             # at once: nothing stepped here may reach the file
    sim.output_drain()
    check_async_file(B, A, sim)
    res = pkg.LbmDem.checkpoint_load(B)
    assert res.nbsteps == n1
    res.renderScene(60)
    same_restart(sim, res)
    sim.close(); res.close()


# ---- 3. corruption -------------------------------------------------------------------------------------------------------------------

def test_a_corrupted_file_is_refused_naming_the_section(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_async_checkpoint(1)
    sim.renderScene(60)
    good, plain = tmp_path / "good.ckpt", tmp_path / "plain.ckpt"
    sim.checkpoint_save_async(str(good))
    sim.checkpoint_save(str(plain))
    sim.output_drain()
    sim.close()
    data = good.read_bytes()
    body, ent = trailer_of(data)
    spans = section_spans(ent)
    assert spans["nbr"][1] > spans["nbr"][0]
    places = dict(header=8,                                         # the first byte of lid6: the header stays plausible
                  nbr=(spans["nbr"][0] + spans["nbr"][1]) // 2,
                  wallflags=spans["wallflags"][1] - 1,
                  f=(spans["f"][0] + spans["f"][1]) // 2)
    for name, at in places.items():
        bad = bytearray(data)
        bad[at] ^= 0x40
        p = tmp_path / (name + ".ckpt")
        p.write_bytes(bytes(bad))
        for call in (pkg.LbmDem.checkpoint_verify, pkg.LbmDem.checkpoint_load):
            with pytest.raises(pkg.LbmDemError) as e:
                call(str(p))
            assert e.value.code == -1 and f"section '{name}'" in str(e.value), (name, str(e.value))
    cut = tmp_path / "cut.ckpt"
    for keep in (len(data) - 100, len(body) + 20, len(body) + 3):    # inside the entries, the counts, the magic
        cut.write_bytes(data[:keep])
        for call in (pkg.LbmDem.checkpoint_verify, pkg.LbmDem.checkpoint_load):
            with pytest.raises(pkg.LbmDemError) as e:
                call(str(cut))
            assert e.value.code == -1 and "trailer" in str(e.value), str(e.value)
    cut.write_bytes(body)                                            # the trailer dropped whole: the synchronous save's file
    assert body == plain.read_bytes()
    for p in (cut, plain):
        assert pkg.LbmDem.checkpoint_verify(str(p)) is False
        back = pkg.LbmDem.checkpoint_load(str(p))
        assert back.nbsteps == 60
        back.close()
    assert pkg.LbmDem.checkpoint_verify(str(good)) is True
    back = pkg.LbmDem.checkpoint_load(str(good))
    assert back.nbsteps == 60
    back.close()


# ---- 4. the cadence -------------------------------------------------------------------------------------------------------------------

STEPS, FILM, EVERY = 4100, 1300, 900      # VTK frames at 1300, 2600, 3900; the DEM event at 4000; checkpoints at 900 .. 3600
_uninterrupted = {}


def scene_sim(pkg):
    lx, ly, r, x1, x2 = g4()
    phys = pkg.derive(lx, ly, r).phys
    phys.stepFilm = FILM
    return pkg.LbmDem(lx, ly, r, x1, x2, physics=phys)


def uninterrupted(pkg, tmp_path_factory):
    """run A, once for the three cases: its directory, console lines, result and final state"""
    if not _uninterrupted:
        d = tmp_path_factory.mktemp("uninterrupted")
        a = scene_sim(pkg)
        lines, res = a.run_scene(STEPS, outdir=str(d))
        _uninterrupted.update(dir=d, lines=lines, res=res, f=a.f, obst=a.obst, kin=a.kinematics, fhf=a.fhf, gp=a.grain_pressure)
        a.close()
    return _uninterrupted


@pytest.mark.parametrize("mode", ["slots", "synchronous", "with_async_output_and_dem"])
def test_run_scene_saves_on_the_cadence_and_changes_nothing_else(pkg, tmp_path, tmp_path_factory, mode):
    A = uninterrupted(pkg, tmp_path_factory)
    db, dc = tmp_path / "b", tmp_path / "c"
    db.mkdir(); dc.mkdir()
    ck = tmp_path / "run.ckpt"
    b = scene_sim(pkg)
    if mode != "synchronous":
        b.set_async_checkpoint(1)
    if mode == "with_async_output_and_dem":
        b.set_async_output(2); b.set_async_dem(2)
    b.set_checkpoint_every(EVERY, str(ck))
    lb, rb = b.run_scene(STEPS, outdir=str(db))
    assert rb == A["res"] and rb["steps_done"] == STEPS and rb["nfile"] == 3
    assert without_clock(lb) == without_clock(A["lines"])
    names = sorted(p.name for p in A["dir"].iterdir())
    assert names == sorted(p.name for p in db.iterdir()) and "DEM000003.dat" in names and len(names) == 18, names
    for n in names:
        assert (A["dir"] / n).read_bytes() == (db / n).read_bytes(), n
    for key, got in (("f", b.f), ("obst", b.obst), ("kin", b.kinematics), ("fhf", b.fhf), ("gp", b.grain_pressure)):
        assert np.array_equal(A[key], got), key
    st = b.output_stats_checkpoint()
    want = STEPS // EVERY if mode != "synchronous" else 0
    assert (st["queued"], st["written"], st["failed"]) == (want, want, 0), st      # taken right after the call: drained
    assert pkg.LbmDem.checkpoint_verify(str(ck)) is (mode != "synchronous")
    no_tmp_files(tmp_path)
    b.close()
    # C: the checkpoint holds the last multiple of the cadence; the remainder from there
    last = STEPS // EVERY * EVERY
    c = pkg.LbmDem.checkpoint_load(str(ck))
    assert c.nbsteps == last
    lc, rc = c.run_scene(STEPS - last, outdir=str(dc))
    assert rc["steps_done"] == STEPS - last and rc["nfile"] == 3
    for key, got in (("f", c.f), ("obst", c.obst), ("kin", c.kinematics), ("fhf", c.fhf), ("gp", c.grain_pressure)):
        assert np.array_equal(A[key], got), key
    tail = sorted(p.name for p in dc.iterdir() if p.name.endswith(".vtk") or re.fullmatch(r"DEM\d{6}\.dat", p.name))
    assert tail == sorted(["%s_%06d.vtk" % (f, 2) for f in FIELDS] + ["DEM000003.dat"]), tail
    for n in tail:
        assert (A["dir"] / n).read_bytes() == (dc / n).read_bytes(), n
    c.close()


# ---- 5. back-pressure -------------------------------------------------------------------------------------------------------------------

def test_one_slot_never_drops_a_checkpoint(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_async_checkpoint(1)
    for k in range(3):
        sim.renderScene(17)
        sim.checkpoint_save_async(str(tmp_path / f"{k}.async"))
        sim.checkpoint_save(str(tmp_path / f"{k}.sync"))
    sim.renderScene(17)
    sim.output_drain()
    for k in range(3):
        check_async_file(str(tmp_path / f"{k}.async"), str(tmp_path / f"{k}.sync"), sim)
    st = sim.output_stats_checkpoint()
    assert (st["queued"], st["written"], st["failed"]) == (3, 3, 0)
    assert 0 <= st["slot_waits"] <= 2 and (st["slot_waits"] == 0) == (st["ms_slot_wait"] == 0.0)
    assert st["ms_io"] > 0.0 and st["ms_hold"] > 0.0
    no_tmp_files(tmp_path)
    sim.set_async_checkpoint(2)            # a change of the number of slots keeps nothing and loses nothing
    assert sim.output_stats_checkpoint()["queued"] == 0
    sim.checkpoint_save_async(str(tmp_path / "3.async")); sim.checkpoint_save(str(tmp_path / "3.sync"))
    sim.set_async_checkpoint(0)            # drains
    check_async_file(str(tmp_path / "3.async"), str(tmp_path / "3.sync"), sim)
    sim.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------

def test_a_writer_failure_reaches_the_caller_and_the_handle_goes_on(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    a, b = pkg.LbmDem(lx, ly, r, x1, x2), pkg.LbmDem(lx, ly, r, x1, x2)
    b.set_async_checkpoint(1)
    a.renderScene(24); b.renderScene(24)
    earlier = tmp_path / "earlier.ckpt"
    b.checkpoint_save_async(str(earlier))
    b.output_drain()
    kept = earlier.read_bytes()
    missing = str(tmp_path / "not" / "there" / "x.ckpt")
    a.renderScene(12); b.renderScene(12)
    b.checkpoint_save_async(missing)              # queued: the failure is the writer's
    with pytest.raises(pkg.LbmDemError) as e:
        b.output_drain()
    assert e.value.code == -1 and missing in str(e.value) and "checkpoint" in str(e.value)
    st = b.output_stats_checkpoint()
    assert (st["queued"], st["written"], st["failed"]) == (2, 1, 1)
    b.output_drain()                              # reported once
    b.checkpoint_save_async(missing)              # ... or at the next call, which then queues nothing
    b.renderScene(1); a.renderScene(1)
    with pytest.raises(pkg.LbmDemError) as e:
        while True:                               # (the writer may not have failed yet when the first call looks)
            b.checkpoint_save_async(str(tmp_path / "never.ckpt"))
            b.output_drain()
    assert missing in str(e.value)
    assert earlier.read_bytes() == kept and pkg.LbmDem.checkpoint_verify(str(earlier)) is True
    no_tmp_files(tmp_path)
    # the handle steps and writes a good checkpoint
    a.renderScene(24); b.renderScene(24)
    b.output_drain()
    b.checkpoint_save_async(str(tmp_path / "later.ckpt")); a.checkpoint_save(str(tmp_path / "later.sync"))
    b.output_drain()
    check_async_file(str(tmp_path / "later.ckpt"), str(tmp_path / "later.sync"), b)
    # destroy with a job pending leaves a complete file
    b.renderScene(5); a.renderScene(5)
    b.checkpoint_save_async(str(tmp_path / "last.ckpt")); a.checkpoint_save(str(tmp_path / "last.sync"))
    b.close(); a.close()
    check_async_file(str(tmp_path / "last.ckpt"), str(tmp_path / "last.sync"))
    assert pkg.LbmDem.checkpoint_verify(str(tmp_path / "last.ckpt")) is True
    no_tmp_files(tmp_path)


# ---- 7. refusals, and the handles that are allowed --------------------------------------------------------------------------------------

def test_refusals(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    ck = str(tmp_path / "x.ckpt")
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    with pytest.raises(pkg.LbmDemError) as e:
        sim.checkpoint_save_async(ck)                      # off by default
    assert e.value.code == -1 and "lbmdem_set_async_checkpoint" in str(e.value)
    assert sim.output_stats_checkpoint()["queued"] == 0
    for slots in (-1, 3):
        with pytest.raises(pkg.LbmDemError) as e:
            sim.set_async_checkpoint(slots)
        assert e.value.code == -1
    with pytest.raises(pkg.LbmDemError):
        sim.set_checkpoint_every(-5, ck)
    with pytest.raises(pkg.LbmDemError):
        sim.set_checkpoint_every(100, None)
    sim.set_async_checkpoint(2)
    sim.set_async_checkpoint(0)
    with pytest.raises(pkg.LbmDemError):
        sim.checkpoint_save_async(ck)
    sim.set_async_checkpoint(1)
    with pytest.raises(pkg.LbmDemError) as e:
        sim.dist_enable()
    assert e.value.code == -1
    sim.set_async_checkpoint(0)
    sim.set_checkpoint_every(100, ck)
    with pytest.raises(pkg.LbmDemError) as e:
        sim.dist_enable()
    assert e.value.code == -1
    sim.set_checkpoint_every(0)
    sim.close()
    strip = pkg.LbmDem(lx, ly, r, x1, x2, strip=(0, 128), halo=2)
    dist = pkg.LbmDem(lx, ly, r, x1, x2)
    dist.dist_enable()
    for other in (strip, dist):
        with pytest.raises(pkg.LbmDemError) as e:
            other.set_async_checkpoint(1)
        assert e.value.code == -1
        with pytest.raises(pkg.LbmDemError) as e:
            other.set_checkpoint_every(100, ck)
        assert e.value.code == -1
        other.close()
    sp = pkg.LbmDem(lx, ly, r, x1, x2, precision="f32")    # the float build has no checkpoints at all
    for call in (lambda: sp.set_async_checkpoint(1), lambda: sp.checkpoint_save_async(ck), lambda: sp.set_checkpoint_every(100, ck)):
        with pytest.raises(pkg.LbmDemError) as e:
            call()
        assert e.value.code == -1
    sp.close()
    assert list(tmp_path.iterdir()) == []


def test_a_checkpoint_does_not_carry_the_settings(pkg, tmp_path):
    lx, ly, r, x1, x2 = g4()
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_async_checkpoint(1)
    sim.set_checkpoint_every(10, str(tmp_path / "never.ckpt"))
    sim.renderScene(12)
    sim.checkpoint_save_async(str(tmp_path / "ck"))
    sim.output_drain()
    back = pkg.LbmDem.checkpoint_load(str(tmp_path / "ck"))
    with pytest.raises(pkg.LbmDemError):
        back.checkpoint_save_async(str(tmp_path / "ck2"))
    back.run_scene(25)                                      # no cadence either
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ck"]
    sim.close(); back.close()


@pytest.mark.parametrize("kind", ["vib", "probe"])
def test_vibrating_and_probing_handles_restart_bit_equal(pkg, tmp_path, kind):
    lx, ly, r, x1, x2 = _vib_inputs("G4")
    phys = _shaker(pkg, lx, ly, r)
    a = pkg.LbmDem(lx, ly, r, x1, x2, physics=phys if kind == "vib" else None)
    if kind == "vib":
        a.set_vibration(True)
    else:
        a.probe_enable(every=1, capacity=64, pressure_row=2, points=[(5, 5)])
    a.set_async_checkpoint(1)
    a.renderScene(50)
    A, B = str(tmp_path / "sync.ckpt"), str(tmp_path / "async.ckpt")
    a.checkpoint_save_async(B)
    a.checkpoint_save(A)
    a.renderScene(50)
    a.output_drain()
    check_async_file(B, A, a)
    res = pkg.LbmDem.checkpoint_load(B)
    assert res.vibrating == (kind == "vib")
    res.renderScene(50)
    same_restart(a, res)
    if kind == "vib":
        assert a.walls() == res.walls()
    a.close(); res.close()


# ---- 8. a replayed run -----------------------------------------------------------------------------------------------------------------

GIVEUP_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import __graft_entry__ as ge, samples
pkg = ge.load_package()
out = sys.argv[1]
lx, ly = 512, 320
r, x, y = samples.row_packing(lx, ly, 700, seed=5)
r, x1, x2 = samples.to_metres(r, x, y)
a = pkg.LbmDem(lx, ly, r, x1, x2)          # the multi-sub-step kernel, one launch made to give up
b = pkg.LbmDem(lx, ly, r, x1, x2); b.set_dem_chain(0)
k = a.kinematics
k[:, 3:6] = np.random.default_rng(17).normal(0, 1, (len(r), 3)) * (0.05, 0.05, 30.0)
a.kinematics = k; b.kinematics = k
pa, pb = os.path.join(out, "a.ckpt"), os.path.join(out, "b.ckpt")
for s, p in ((a, pa), (b, pb)):
    s.set_async_checkpoint(1)
    s.set_checkpoint_every(90, p)
a.debug_chain_giveup(3)        # inside the first stretch: the checkpoint of step 90 is the call that finds it
la, ra = a.run_scene(345)
lb, rb = b.run_scene(345)
assert a.dem_chain_recoveries() == 1 and b.dem_chain_recoveries() == 0
assert ra == rb and ra["steps_done"] == 345
for s in (a, b):
    st = s.output_stats_checkpoint()
    assert (st["queued"], st["written"], st["failed"]) == (3, 3, 0), st
da, db = open(pa, "rb").read(), open(pb, "rb").read()
assert da == db and pkg.LbmDem.checkpoint_verify(pa) is True
c = pkg.LbmDem.checkpoint_load(pa)
assert c.nbsteps == 270
c.renderScene(75)
assert np.array_equal(a.f, b.f) and np.array_equal(a.kinematics, b.kinematics) and np.array_equal(a.obst, b.obst)
assert np.array_equal(a.f, c.f) and np.array_equal(a.kinematics, c.kinematics) and np.array_equal(a.obst, c.obst)
a.close(); b.close(); c.close()
print("recovered: checkpoint bytes", len(da))
"""


def test_a_replayed_run_writes_the_checkpoint_of_the_undisturbed_one(tmp_path):
    """A launch of the multi-sub-step DEM kernel that gives up (made to, in the experiment build, as
    tests/test_gpu_async_output.py::test_a_replayed_run_writes_the_frames_of_the_undisturbed_one does) before a cadence
    checkpoint: the save settles the handle first -- the launch is undone, its sub-steps repeated -- and only then snapshots."""
    lib = os.path.join(ROOT, "2d-lbm-dem_amd", "liblbmdem_hip_ab.so")
    assert os.path.exists(lib), "run __graft_entry__.build()"
    env = dict(os.environ, LBMDEM_HIP_LIBRARY=lib)
    out = subprocess.run([sys.executable, "-c", GIVEUP_SCRIPT, str(tmp_path)], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "recovered: checkpoint bytes" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 9. the host driver ------------------------------------------------------------------------------------------------------------------

def test_host_driver_periodic_checkpoints(po, tmp_path):
    c = gu.CASES["G4_coupled_256x200"]

    def drive(d, args):
        d.mkdir(exist_ok=True)
        sample = d / "packing.data"
        if not sample.exists():
            po.write_sample(str(sample), c["r_mm"], c["x_mm"], c["y_mm"])
        out = subprocess.run([EXE, str(sample), "--lx", "256", "--ly", "200"] + args, capture_output=True, text=True, cwd=d,
                             timeout=900)
        assert out.returncode == 0, (out.stdout[-400:], out.stderr[-1200:])
        return out

    fd = lambda o: re.search(r"^final_density: ([0-9.]+)$", o.stderr, re.M).group(1)
    console = lambda o: [l.split(" Time ")[0] for l in o.stdout.splitlines() if l.startswith(("Iteration Number", "steps "))]
    plain = drive(tmp_path / "plain", ["--steps", "4100", "--checkpoint", "run.ckpt"])
    every = drive(tmp_path / "every", ["--steps", "4100", "--checkpoint", "run.ckpt", "--checkpoint-every", "1500",
                                       "--async-checkpoint", "--run-stats"])
    names = sorted(p.name for p in (tmp_path / "plain").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "every").iterdir()) and "DEM000000.dat" in names, names
    for n in names:
        if n != "run.ckpt":
            assert (tmp_path / "plain" / n).read_bytes() == (tmp_path / "every" / n).read_bytes(), n
    check_async_file(str(tmp_path / "every" / "run.ckpt"), str(tmp_path / "plain" / "run.ckpt"))
    assert fd(plain) == fd(every) and console(plain) == console(every) and len(console(plain)) >= 40
    m = re.search(r"^async_checkpoint: queued (\d+) written (\d+) failed (\d+) ", every.stderr, re.M)
    assert m and [int(v) for v in m.groups()] == [3, 3, 0], every.stderr[-800:]      # 1500, 3000, the final one
    assert "async_checkpoint" not in plain.stderr
    # a run that ends at a periodic checkpoint, restarted: the tail of the uninterrupted run
    drive(tmp_path / "tail", ["--steps", "3000", "--checkpoint", "run.ckpt", "--checkpoint-every", "1500", "--async-checkpoint"])
    stats_before = (tmp_path / "tail" / "stats.data").read_bytes()
    tail = drive(tmp_path / "tail", ["--restart", "run.ckpt", "--steps", "4100"])
    assert "Restarted from run.ckpt at step 3000" in tail.stdout
    assert fd(tail) == fd(plain)
    assert (tmp_path / "tail" / "DEM000000.dat").read_bytes() == (tmp_path / "plain" / "DEM000000.dat").read_bytes()
    assert (tmp_path / "tail" / "stats.data").read_bytes().startswith(stats_before)
    no_tmp_files(tmp_path)
    # --verify-checkpoint: no device, exit status
    good = tmp_path / "every" / "run.ckpt"
    ok = subprocess.run([EXE, "--verify-checkpoint", str(good)], capture_output=True, text=True, timeout=120)
    assert ok.returncode == 0 and "matches" in ok.stdout, (ok.stdout, ok.stderr)
    bad = tmp_path / "flipped.ckpt"
    data = bytearray(good.read_bytes())
    data[len(data) // 2] ^= 1
    bad.write_bytes(bytes(data))
    no = subprocess.run([EXE, "--verify-checkpoint", str(bad)], capture_output=True, text=True, timeout=120)
    assert no.returncode != 0 and "section 'f'" in no.stderr, (no.stdout, no.stderr)
    # --checkpoint-every needs --checkpoint, and a single GPU
    for args in (["--checkpoint-every", "100"], ["--checkpoint", "x", "--checkpoint-every", "100", "--gpus", "2"]):
        out = subprocess.run([EXE, str(tmp_path / "plain" / "packing.data"), "--lx", "256", "--ly", "200", "--steps", "10"] + args,
                             capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert out.returncode != 0 and "--checkpoint" in out.stderr, (out.stdout, out.stderr)
