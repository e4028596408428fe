#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the UNMODIFIED reference.

Runs only in the build container, where /root/reference exists: oracle/ref_harness.c compiles the
reference's src/main.c (one library per lattice size, -O2 -ffp-contract=off) and this script drives
it. What is committed is data only -- the inputs we authored (grain radii/positions in the
reference's .data units, initial perturbation seeds) and the reference's outputs -- never the
reference's source.

    python tests/golden/make_golden.py            # regenerate every fixture
    python tests/golden/make_golden.py --shapes   # only the odd-shape cases S_* (fp64 and float) and vtk_S_61x59/
    python tests/golden/make_golden.py --packed   # only the packed case P_tri_127x121 (fp64 and float)

Each case runs in its own process (the reference keeps its state in file-scope globals).
Large arrays are stored as a strided sample plus the SHA-256 of the full little-endian float64
buffer, which pins every bit while keeping the repository small.
"""
import hashlib
import multiprocessing as mp
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def perturbation(lx, ly, seed, amp):
    """Smooth + random multiplicative perturbation of f (applied to whatever f currently is)."""
    rng = np.random.default_rng(seed)
    x = np.arange(lx)[:, None, None] / lx
    y = np.arange(ly)[None, :, None] / ly
    smooth = 0.02 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) * np.linspace(-1, 1, 9)[None, None, :]
    return 1.0 + smooth + amp * rng.standard_normal((lx, ly, 9))


# ---- case definitions (shared with the tests through cases()) ---------------------------------------

def cases():
    import samples
    c = {}
    # G1: (almost) fluid-only -- the reference cannot run with 0 grains (main.c:220), so one small
    # grain sits in a corner; f starts from a smooth + noisy perturbation. Fluid phases only.
    for name, lx, ly in (("G1_fluid_64x48", 64, 48), ("G1_fluid_128x128", 128, 128)):
        c[name] = dict(kind="lbm", lx=lx, ly=ly, r_mm=[0.5], x_mm=[1.2], y_mm=[1.1], kin=None,
                       pert=(101, 1e-3), dumps=(1, 10, 50))
    # G2: one translating + spinning grain -> reinit, both delta branches, moving-wall term, fhf
    c["G2_moving_grain_96x96"] = dict(kind="lbm", lx=96, ly=96, r_mm=[0.85], x_mm=[4.63], y_mm=[4.21],
                                      kin=[[0.03, -0.02, 40.0]], pert=(202, 1e-3), dumps=(1, 5, 20),
                                      drift=[[2.3e-5, -1.7e-5]])
    # G3: two grains one fluid node apart -> the in-place IBB order hazard (SURVEY.md hard part 2)
    dx = 0.1 * 96 / 95
    d = 0.85 * (0.7 + 0.6) + 1.6 * dx
    ang = 0.25 * np.pi
    c["G3_hazard_96x96"] = dict(kind="lbm", lx=96, ly=96, r_mm=[0.7, 0.6],
                                x_mm=[4.0, 4.0 + d * np.cos(ang)], y_mm=[4.2, 4.2 + d * np.sin(ang)],
                                kin=[[0.01, -0.015, 15.0], [-0.02, 0.01, -25.0]], pert=(303, 1e-2),
                                dumps=(1, 2, 3))
    # G4: ~600-grain packing, fully coupled, 20 fluid steps
    r, x, y = samples.row_packing(256, 200, 600, seed=77)
    c["G4_coupled_256x200"] = dict(kind="coupled", lx=256, ly=200, r_mm=r, x_mm=x, y_mm=y, fluid_steps=20)
    # G6: output files. G4's packing plus four grains pressed into the DEM walls, 4000 renderScene calls:
    # the reference then writes DEM000000.dat and appends a line to stats.data (main.c:1773-1776)
    r, x, y = samples.row_packing(256, 200, 600, seed=77)
    r = np.concatenate([r, [0.6, 0.7, 0.8, 0.9]])
    x = np.concatenate([x, [0.6 - 0.002, 60.0, 256 - 0.8 + 0.002, 80.0]])
    y = np.concatenate([y, [90.0, 0.7 - 0.003, 40.0, 200 - 0.9 + 0.003]])
    c["G6_output_256x200"] = dict(kind="output", lx=256, ly=200, r_mm=r, x_mm=x, y_mm=y, steps=4000)
    # G5: DEM-focused: 240 renderScene calls on a tiny lattice with random initial grain velocities:
    # film law at step 0, Verlet rebuilds at 0/100/200, grain-grain contacts, and four extra grains
    # pressed 2-3 um into the left/bottom/right/top DEM walls (the right/top walls sit at 1e-3*lx,
    # 1e-3*ly metres after the first VerletWall, main.c:1559-1560 -- outside the lattice).
    r, x, y = samples.row_packing(64, 48, 14, seed=9)
    r = np.concatenate([r, [0.6, 0.7, 0.8, 0.9]])
    x = np.concatenate([x, [0.6 - 0.002, 20.0, 64 - 0.8 + 0.002, 30.0]])
    y = np.concatenate([y, [30.0, 0.7 - 0.003, 10.0, 48 - 0.9 + 0.003]])
    c["G5_dem_64x48"] = dict(kind="dem", lx=64, ly=48, r_mm=r, x_mm=x, y_mm=y, seed=505, dumps=(1, 120, 240))
    # S: odd and ragged lattice shapes, fully coupled and agitated. lx % 8 = 1 ... 7 (a last segment of the fused kernel's row
    # march that is short, down to one row) and ly % 60 in {0, 1, 2, 3, 17, 59} (a last 60-column window that produces the wall
    # column alone, one or two interior columns and the wall, or is one column short of full); ly is no multiple of 16 or 32
    # (the padded row pitch of the double and of the float build). Where the lattice is at least 60 nodes wide (lx >= 60: all but
    # 13 x 61 and 33 x 62, which hold six grains each), grains 0-3 are pushed into the left, bottom, right and top walls so that
    # the lattice clamp clips a disc at every edge.
    for lx, ly in SHAPES:
        seed = SHAPE_SEEDS.get((lx, ly), 1000 * lx + ly)
        r, x, y = samples.row_packing(lx, ly, 400, seed=seed, margin=0.05)
        if len(r) < 3:       # 13 rows = 1.3 mm: only small grains fit
            r, x, y = samples.row_packing(lx, ly, 400, seed=seed, margin=0.05, rmin=0.3, rmax=0.45)
        elif lx >= 60:
            x[0], y[1], x[2], y[3] = 0.35, 0.35, 0.1 * lx - 0.35, 0.1 * ly - 0.35
        c[f"S_{lx}x{ly}"] = dict(kind="shape", lx=lx, ly=ly, r_mm=r, x_mm=x, y_mm=y, seed=7, dumps=SHAPE_DUMPS)
    # P: a two-dimensional packing (tests/packing_util.py: a jittered triangular lattice, 156 grains numbered at random), run and
    # dumped like the S cases. Rows never touch each other; here more than half of the grains carry three or more non-zero
    # contact forces and two thirds of the contact normals are steep: the sums of force_grains' `double fn, ft` over several
    # partners, in both precisions.
    import packing_util
    r, x, y = packing_util.tri_packing(127, 121, 0.5, shuffle=True)
    c["P_tri_127x121"] = dict(kind="shape", lx=127, ly=121, r_mm=r, x_mm=x, y_mm=y, seed=7, dumps=SHAPE_DUMPS,
                              file_max=58405)      # no larger than the largest S_*.npz (S_98x119)
    return c


SHAPES = ((13, 61), (33, 62), (61, 59), (67, 60), (98, 119), (100, 63), (126, 77), (127, 121), (75, 183), (203, 122))
SHAPE_SEEDS = {(61, 59): 61061}     # 1000 lx + ly packs 10 grains there; the checkpoint tests want an odd count (11)
SHAPE_DUMPS = (1, 3, 6)      # whole fluid periods (npDEM sub-steps each); the run ends 5 sub-steps after the last


def kin_table(case):
    r_mm = np.asarray(case["r_mm"], float)
    n = len(r_mm)
    k = np.zeros((n, 9))
    k[:, 0] = np.asarray(case["x_mm"], float) * 1e-3
    k[:, 1] = np.asarray(case["y_mm"], float) * 1e-3
    if case.get("kin") is not None:
        k[:, 3:6] = np.asarray(case["kin"], float)
    return k


def dem_initial_kinematics(case):
    k = kin_table(case)
    rng = np.random.default_rng(case["seed"])
    k[:, 3:6] = rng.normal(0, 1, (len(k), 3)) * [0.05, 0.05, 30.0]
    return k


def shape_initial_kinematics(case):
    k = kin_table(case)
    rng = np.random.default_rng(case["seed"])
    k[:, 3:6] = rng.normal(0, 1, (len(k), 3)) * [0.3, 0.3, 40.0]
    return k


# ---- drivers (work on anything with the Reference/Oracle interface) ---------------------------------

def run_lbm_case(sim, case):
    """-> dict of dumps. `sim` has set_f/get_f/set_kinematics/lbm_steps/get_obst/get_fhf."""
    lx, ly = case["lx"], case["ly"]
    k = kin_table(case)
    sim.set_kinematics(k)
    f0 = sim.get_f() * perturbation(lx, ly, *case["pert"])
    sim.set_f(f0)
    out = {}
    done = 0
    for target in case["dumps"]:
        while done < target:
            if case.get("drift") is not None:
                k[:, 0:2] += np.asarray(case["drift"], float)
                sim.set_kinematics(k)
            sim.lbm_steps(1)
            done += 1
        out[f"f_{target}"] = sim.get_f()
        out[f"obst_{target}"] = sim.get_obst()
        out[f"fhf_{target}"] = sim.get_fhf()
    return out


def run_coupled_case(sim, case):
    npdem = sim.scalars()["npDEM"]
    sim.steps(case["fluid_steps"] * npdem)
    return {"f": sim.get_f(), "obst": sim.get_obst(), "fhf": sim.get_fhf(), "grains": sim.get_grains()}


def run_dem_case(sim, case):
    sim.set_kinematics(dem_initial_kinematics(case))
    out = {}
    done = 0
    for target in case["dumps"]:
        sim.steps(target - done)
        done = target
        out[f"grains_{target}"] = sim.get_grains()
    out["f_final"] = sim.get_f()
    return out


def run_shape_case(sim, case):
    """6 npDEM + 5 sub-steps from agitated grains. After 1, 3 and 6 fluid periods and at the end ("end"): SHA-256 of f, obst,
    fhf and the kinematics, and the serial total density; at the end the arrays themselves as well. `sim` has
    set_kinematics/steps/get_f/get_obst/get_fhf/get_grains/total_density/scalars."""
    sim.set_kinematics(shape_initial_kinematics(case))
    npdem = sim.scalars()["npDEM"]
    out = {}
    done = 0
    for d in tuple(case["dumps"]) + ("end",):
        target = case["dumps"][-1] * npdem + 5 if d == "end" else d * npdem
        sim.steps(target - done)
        done = target
        f, obst, fhf, grains = sim.get_f(), sim.get_obst(), sim.get_fhf(), sim.get_grains()
        out[f"sha_f_{d}"] = sha(f)
        out[f"sha_obst_{d}"] = sha(np.asarray(obst).astype(np.int32))
        out[f"sha_fhf_{d}"] = sha(fhf)
        out[f"sha_kin_{d}"] = sha(grains[:, :9])
        out[f"density_{d}"] = np.float64(sim.total_density())
    out.update(f_end=f, obst_end=obst, fhf_end=fhf, grains_end=grains)
    return out


def _reference(name, case, sp=False):
    import pyoracle as po
    tmp = tempfile.NamedTemporaryFile("w", suffix=".data", delete=False)
    tmp.close()
    po.write_sample(tmp.name, case["r_mm"], case["x_mm"], case["y_mm"], comment=f"#golden {name}")
    R = po.Reference(case["lx"], case["ly"], tmp.name, sp=sp)      # sp: the reference compiled -DSINGLE_PRECISION (main.c:34-40)
    os.unlink(tmp.name)
    return R


def _generate(name, case, q, sp=False):
    import pyoracle as po
    R = _reference(name, case, sp)
    if case["kind"] == "lbm":
        res = run_lbm_case(R, case)
    elif case["kind"] == "coupled":
        res = run_coupled_case(R, case)
    elif case["kind"] == "shape":
        res = run_shape_case(R, case)
    else:
        res = run_dem_case(R, case)
    res["scalars"] = np.array([R.scalars()[k] for k in po.SCALARS], float)
    q.put(res)


SHAPE_FILE_MAX = 65536      # shape cases: a fixture file stays below this; the f sample is the first thing to go


def pack(name, case, res, f_sample=True):
    """Reduce a result dict to what is stored. Shape cases: f as a strided sample whatever the lattice size (f_sample = False:
    its digest alone, for a file that would not stay under SHAPE_FILE_MAX with it); the obstacle map in full."""
    shape = case["kind"] == "shape"
    out = {"r_mm": np.asarray(case["r_mm"], float), "x_mm": np.asarray(case["x_mm"], float),
           "y_mm": np.asarray(case["y_mm"], float), "scalars": res["scalars"]}
    for k, v in res.items():
        if k == "scalars":
            continue
        if isinstance(v, str):
            out[k] = np.array(v)
            continue
        v = np.asarray(v)
        out[k + "_sha"] = np.array(sha(v))
        if shape and v.ndim == 3:
            if f_sample:
                out[k + "_sample"] = v[::4, ::4, :].copy()
        elif shape:
            out[k] = v
        elif v.ndim == 3 and v.shape[0] * v.shape[1] > 64 * 48:      # big f dump: strided sample
            out[k + "_sample"] = v[::4, ::4, :].copy()
        elif v.ndim == 2 and v.dtype.kind == "i" and v.size > 64 * 48:
            out[k + "_sample"] = v[::4, ::4].copy()
        else:
            out[k] = v
    return out


VTK_NFILE = 3


def make_vtk_fixture(name="G5_dem_64x48"):
    """tests/golden/vtk_G5_25steps/*.vtk: the five files the reference's write_vtk (main.c:237-338)
    produces for case G5 after 25 renderScene calls with nFile = 3 (data written by the reference).
    For a shape case, tests/golden/vtk_<case>/: the same five files after the case's last dump."""
    c = cases()[name]
    R = _reference(name, c)
    if c["kind"] == "shape":
        run_shape_case(R, c)
        out = os.path.join(HERE, "vtk_" + name)
    else:
        R.set_kinematics(dem_initial_kinematics(c))
        R.steps(25)
        out = os.path.join(HERE, "vtk_G5_25steps")
    os.makedirs(out, exist_ok=True)
    assert R.L.ref_write_vtk(os.fsencode(out), VTK_NFILE) == 0


def make_vtk_shape_fixture():
    make_vtk_fixture("S_61x59")


def make_dry_output_fixture():
    """tests/golden/dem_dry_G6_4000steps/: the same files from the reference compiled WITHOUT `_FLUIDE_` (main.c:16 taken out:
    oracle/Makefile ref_dry) -- its DEM-only mode: no fluid step, no VTK frames, hydrodynamic forces 0 (main.c:1709-1719,
    1768-1772)."""
    make_dem_output_fixture(dry=True)


def make_dem_output_fixture(dry=False):
    """tests/golden/dem_G6_4000steps/{DEM000000.dat, stats.data}: what the reference's write_DEM
    (main.c:340-438) writes for case G6 at step 4000, plus the grain table at that moment."""
    import ctypes
    import pyoracle as po
    c = cases()["G6_output_256x200"]
    tmp = tempfile.NamedTemporaryFile("w", suffix=".data", delete=False)
    tmp.close()
    po.write_sample(tmp.name, c["r_mm"], c["x_mm"], c["y_mm"])
    R = po.Reference(c["lx"], c["ly"], tmp.name, dry=dry)
    os.unlink(tmp.name)
    out = os.path.join(HERE, "dem_dry_G6_4000steps" if dry else "dem_G6_4000steps")
    os.makedirs(out, exist_ok=True)
    for f in os.listdir(out):
        os.unlink(os.path.join(out, f))
    assert R.L.ref_steps_in_dir(ctypes.c_long(c["steps"]), os.fsencode(out)) == 0
    # write_forces' PostScript picture (main.c:440-478). Three header lines come from undefined printf
    # conversions ("%%%BoundingBox" ...) and the (nbgrains+1)-th grain line from g[nbgrains], one element
    # past the array: dropped here; every other line is kept as the fixture.
    ps = os.path.join(out, "DEM000000.ps")
    lines = open(ps, "rb").read().split(b"\n")
    n = len(c["r_mm"])
    assert lines[0].startswith(b"%!PS-Adobe") and lines[4].startswith(b"0.1 setlinewidth")
    assert all(l.startswith(b"newpath ") for l in lines[5:5 + n + 1])
    kept = [lines[0], lines[4]] + lines[5:5 + n] + lines[5 + n + 1:]
    open(ps, "wb").write(b"\n".join(kept))
    np.savez_compressed(os.path.join(out, "inputs_and_table.npz"), r_mm=np.asarray(c["r_mm"], float),
                        x_mm=np.asarray(c["x_mm"], float), y_mm=np.asarray(c["y_mm"], float),
                        grains=R.get_grains())


# ---- the reference's own sample inputs at BASELINE.json's sizes ----------------------------------------

REAL_CASES = {
    # name: (sample file under /root/reference/bin, lx, ly, fluid steps at which the state is hashed)
    "real_a08d83_600x500": ("a08d83.data", 600, 500, (1, 10, 20)),             # SURVEY.md section 8c known answers
    "real_7000_2048x2048": ("a08_a4b4r18_7000.data", 2048, 2048, (1, 2, 50)),  # BASELINE.json configs[2]
    "real_50000_4096x4096": ("50000.data", 4096, 4096, (1, 2, 10, 20, 100)),       # BASELINE.json configs[3]
    "real_50000test_3072x3072": ("50000-test.data", 3072, 3072, (1, 2, 30)),   # BASELINE.json configs[0] (47 980 grains)
    "real_50000_8192x4096": ("50000.data", 8192, 4096, (1, 2, 10, 20)),        # BASELINE.json configs[4] (one domain = 8 strips)
    # the JUBE cases of the reference's own benchmark.xml (lines 7, 13-27) at scale 1, and the remaining shipped samples
    "real_a08d83_2000x1000": ("a08d83.data", 2000, 1000, (1, 2, 10)),
    "real_a6d83_2000x1000": ("a6d83.data", 2000, 1000, (1, 2, 10)),            # grains up to y = 1493 nodes: outside the lattice
    "real_slope_12500x2500": ("slope.data", 12500, 2500, (1, 2, 10)),          # r up to 1.5 mm (12.8 nodes reduced)
    "real_spl04_1600x2400": ("spl04.data", 1600, 2400, (1, 2, 10)),            # = 10000_before_packing.data, 9 984 grains
}
# fixtures that do not repeat the parsed grains of another fixture of the same sample file (r, x1, x2 are the same
# doubles: read_sample does not depend on the lattice)
GRAINS_FROM = {"real_50000_8192x4096": "real_50000_4096x4096"}


F32_REAL_CASES = {"real_a08d83_600x500_f32": ("a08d83.data", 600, 500, (1, 10, 20))}


def _real_case(name, q, sp=False):
    """Runs in its own process: the reference on one of its shipped samples; returns the parsed grains
    (exactly the doubles the reference works with) and SHA-256 digests of its state."""
    import pyoracle as po
    fname, lx, ly, dumps = (F32_REAL_CASES if sp else REAL_CASES)[name]
    po.build_ref(lx, ly, sp=sp)
    devnull = os.open(os.devnull, os.O_WRONLY)
    os.dup2(devnull, 1)
    R = po.Reference(lx, ly, os.path.join(po.REF_ROOT, "bin", fname), sp=sp)
    g0 = R.get_grains()
    s = R.scalars()
    out = dict(r=g0[:, po.COL["r"]].copy(), x1=g0[:, 0].copy(), x2=g0[:, 1].copy(),
               npDEM=np.int64(s["npDEM"]), dx=np.float64(s["dx"]), c=np.float64(s["c"]), dumps=np.array(dumps))
    if name in GRAINS_FROM:
        other = np.load(os.path.join(HERE, GRAINS_FROM[name] + ".npz"))
        assert all(np.array_equal(out[k], other[k]) for k in ("r", "x1", "x2"))
        for k in ("r", "x1", "x2"):
            del out[k]
        out["grains_from"] = np.array(GRAINS_FROM[name])
    done = 0
    for k in dumps:
        R.steps((k - done) * int(s["npDEM"]))
        done = k
        g = R.get_grains()
        out[f"sha_f_{k}"] = sha(R.get_f())
        out[f"sha_obst_{k}"] = sha(R.get_obst().astype(np.int32))
        out[f"sha_fhf_{k}"] = sha(R.get_fhf())
        out[f"sha_kin_{k}"] = sha(g[:, :9])
        out[f"mass_{k}"] = np.float64(R.total_density())
        out[f"grain0_{k}"] = g[0, :9].copy()
    q.put(out)


def make_real_fixtures(only=None):
    for name in (only or REAL_CASES):
        q = mp.Queue()
        p = mp.Process(target=_real_case, args=(name, q))
        p.start()
        res = q.get()
        p.join()
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **res)
        print("wrote", name, {k: str(v)[:20] for k, v in res.items() if k.startswith(("sha_f", "mass"))})


def make_case_fixtures(sp=False, kinds=None, prefix=""):
    """<case>.npz / <case>_f32.npz for every case (of these kinds, with this prefix) that is stored as one file"""
    for name, case in cases().items():
        if case["kind"] == "output" or (kinds is not None and case["kind"] not in kinds) or not name.startswith(prefix):
            continue
        q = mp.Queue()
        p = mp.Process(target=_generate, args=(name, case, q, sp))
        p.start()
        res = q.get()
        p.join()
        path = os.path.join(HERE, name + ("_f32" if sp else "") + ".npz")
        packed = pack(name, case, res)
        np.savez_compressed(path, **packed)
        file_max = case.get("file_max", SHAPE_FILE_MAX)
        if case["kind"] == "shape" and os.path.getsize(path) >= file_max:      # does not fit: without the f sample
            packed = pack(name, case, res, f_sample=False)
            np.savez_compressed(path, **packed)
            assert os.path.getsize(path) < file_max, (path, os.path.getsize(path))
        print("wrote", os.path.basename(path), os.path.getsize(path), {k: getattr(v, "shape", None) for k, v in packed.items()})


def make_f32_fixtures(kinds=None):
    """<case>_f32.npz: the same cases on the reference compiled -DSINGLE_PRECISION (typedef float real, main.c:34-40):
    the oracle of the float build of the library (liblbmdem_hip_sp.so). Stored as float64 arrays holding float values."""
    make_case_fixtures(sp=True, kinds=kinds)
    if kinds is not None:
        return
    for name in F32_REAL_CASES:
        q = mp.Queue()
        p = mp.Process(target=_real_case, args=(name, q, True))
        p.start()
        res = q.get()
        p.join()
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **res)
        print("wrote", name, {k: str(v)[:20] for k, v in res.items() if k.startswith(("sha_f", "mass"))})


def main():
    import pyoracle as po
    if not po.reference_available():
        raise SystemExit("the reference is not present here; golden vectors can only be made in the build container")
    if len(sys.argv) > 1 and sys.argv[1] == "--f32":
        make_f32_fixtures()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--shapes":     # only the S_* cases, both precisions, and their VTK frame
        make_case_fixtures(kinds=("shape",), prefix="S_")
        make_case_fixtures(sp=True, kinds=("shape",), prefix="S_")
        p = mp.Process(target=make_vtk_shape_fixture)
        p.start()
        p.join()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--packed":
        make_case_fixtures(prefix="P_")
        make_case_fixtures(sp=True, prefix="P_")
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--dry":
        make_dry_output_fixture()
        return
    if len(sys.argv) > 1:      # python make_golden.py real_50000_8192x4096 ...: only these real-sample fixtures
        make_real_fixtures(sys.argv[1:])
        return
    make_case_fixtures()
    make_real_fixtures()
    for target in (make_vtk_fixture, make_vtk_shape_fixture, make_dem_output_fixture, make_dry_output_fixture):
        p = mp.Process(target=target)
        p.start()
        p.join()


if __name__ == "__main__":
    main()
