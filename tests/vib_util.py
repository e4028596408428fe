"""Shared by the vibrating-wall tests: the CPU oracle with the reference's vib = 1 (tests/vib_oracle/vib_oracle.c, built by
__graft_entry__.build()), physics for a shaken box, and packings whose grains touch the left, right and top walls."""
import ctypes as C
import math
import os

import numpy as np

import pyoracle

HERE = os.path.dirname(os.path.abspath(__file__))
VIB_LIB = os.path.join(HERE, "vib_oracle", "libvib_oracle.so")
PHYS_NAMES = ("rho_moy tau s2 s3 s5 s7 s8 s9 nu reductionR G angleG km kg kt ktm nug num nugt "
              "mu mum mumb murf distVerlet dtt iterDEM freq amp t").split()


class VibOracle(pyoracle.Oracle):
    """pyoracle.Oracle over libvib_oracle.so (the oracle's own TU plus main.c:1700-1705 in front of renderScene)."""

    def __init__(self, lx, ly, r, x1, x2, phys=None, scale=1.0):
        if not os.path.exists(VIB_LIB):
            raise RuntimeError(f"{VIB_LIB} not built -- run __graft_entry__.build()")
        orig = pyoracle.build_oracle
        pyoracle.build_oracle = lambda fast=False: VIB_LIB
        try:
            super().__init__(lx, ly, r, x1, x2, scale)
        finally:
            pyoracle.build_oracle = orig
        self.L.vib_get_walls.argtypes = [C.c_void_p, C.c_void_p]
        if phys is not None:
            self.set_physics([getattr(phys, n) for n in PHYS_NAMES], phys.updateVerlet, phys.stepFilm)

    def vib_steps(self, n): self.L.vib_steps(self.h, C.c_long(n))
    def vib_steps_dry(self, n): self.L.vib_steps_dry(self.h, C.c_long(n))

    def walls(self):
        out = np.zeros(5)
        self.L.vib_get_walls(self.h, out.ctypes.data_as(C.c_void_p))
        return dict(zip(("t", "Mgx", "Mdx", "Mby", "Mhy"), (float(v) for v in out)))

    def vib_steps_counting(self, n, contacts, dry=False):
        """n sub-steps one at a time; contacts["left" | "right" | "top"] += 1 for every sub-step in which a grain of that
        wall's candidate list overlaps the wall -- the reference's condition for applying the wall law (main.c:1455-1508),
        with the positions the sub-step's forces were computed from and the walls of that sub-step"""
        step = self.vib_steps_dry if dry else self.vib_steps
        ri = pyoracle.COL["r"]
        for _ in range(n):
            step(1)
            g, w = self.get_grains(), self.walls()
            _, _, _, (_, lt, ll, lr) = self.verlet()
            x1, x2, r = g[:, 0], g[:, 1], g[:, ri]
            contacts["left"] += int(len(ll) > 0 and bool(np.any(x1[ll] - r[ll] - w["Mgx"] < 0)))
            contacts["right"] += int(len(lr) > 0 and bool(np.any(-x1[lr] - r[lr] + w["Mdx"] < 0)))
            contacts["top"] += int(len(lt) > 0 and bool(np.any(-x2[lt] - r[lt] + w["Mhy"] < 0)))


def physics(pkg, freq, amp, dtt=1.0, t=0.0):
    """the reference's initialisers with the shaker's freq, amp; dtt = 1 s keeps VerletWall's resets at the lattice edges
    (main.c:1555-1557: the right and top walls grains can reach)"""
    phys = pkg.Physics()
    pkg.load_library().lbmdem_physics_defaults(C.byref(phys))
    phys.freq, phys.amp, phys.dtt, phys.t = freq, amp, dtt, t
    return phys


def restated_walls(cfg, nbsteps0, n):
    """main.c:1700-1705 and 1555-1561 in Python floats (one rounding per operation, math.sin / math.cos):
    rows t, Mgx, Mdx, amp*freq*cos(freq*t) of sub-steps nbsteps0 .. nbsteps0 + n - 1"""
    p = cfg.phys
    t, Mgx, Mdx = p.t, cfg.Mgx, cfg.Mdx
    rows = []
    for k in range(n):
        step = nbsteps0 + k
        t = t + cfg.dt
        Mgx = Mgx + p.amp * math.sin(p.freq * t)
        Mdx = Mdx + p.amp * math.sin(p.freq * t)
        if step % p.updateVerlet == 0:
            Mdx = 1.e-3 * cfg.lx / 10 if step * cfg.dt < p.dtt else 1.e-3 * cfg.lx
        rows.append((t, Mgx, Mdx, p.amp * p.freq * math.cos(p.freq * t)))
    return np.array(rows)


def with_wall_grains(r, x1, x2, lx, ly, r_new=0.5e-3, overlap=0.02e-3):
    """the packing plus one grain pressed against each of the left, right and top walls (overlap `overlap`), each placed
    where it overlaps no other grain. Metres."""
    W, H = 1e-3 * lx / 10, 1e-3 * ly / 10
    r, x1, x2 = list(r), list(x1), list(x2)

    def free(x, y):
        return all(math.hypot(x - a, y - b) > r_new + c + 1e-5 for a, b, c in zip(x1, x2, r))

    spots = [lambda s: (r_new - overlap, s * H), lambda s: (W - r_new + overlap, s * H), lambda s: (s * W, H - r_new + overlap)]
    for spot in spots:
        for s in np.linspace(0.95, 0.05, 181):
            x, y = spot(s)
            if free(x, y):
                r.append(r_new); x1.append(x); x2.append(y)
                break
        else:
            raise AssertionError("no free place along a wall")
    return np.array(r), np.array(x1), np.array(x2)
