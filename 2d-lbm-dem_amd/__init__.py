"""2d-lbm-dem_amd -- MI355X-native hot path of cb-geo/2d-lbm-dem behind the reference's own seam.

The reference exposes no library API: its seam is the set of ``void fn(void)`` routines that
``renderScene()`` calls on file-scope globals (src/main.c:1697-1777). :class:`LbmDem` mirrors that
seam one-to-one -- same routine names, same call order, same host data layout
(``f[x][y][q]``, x slow) -- on top of the C ABI in ``include/lbmdem_hip.h``
(``liblbmdem_hip.so``, hand-written HIP for gfx950).

There is deliberately NO CPU fallback here: if the HIP library is missing or no GPU is present
every entry point raises. The CPU oracle lives under ``oracle/`` and is test infrastructure only.

The directory name is not a Python identifier; load it with ``importlib`` (see
``__graft_entry__.load_package()``) or put the repo root on ``sys.path`` and use
``importlib.import_module("2d-lbm-dem_amd")``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LBMDEM_HIP_LIBRARY: load another build of the same ABI (e.g. the `make AB=1` experiment build)
LIB_PATH = os.environ.get("LBMDEM_HIP_LIBRARY") or os.path.join(_HERE, "liblbmdem_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lbmdem_hip.h")


class LbmDemError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class Physics(C.Structure):
    """lbmdem_physics -- the initialised globals of main.c:74-118,143,163-165."""
    _fields_ = [(n, C.c_double) for n in (
        "rho_moy tau s2 s3 s5 s7 s8 s9 nu reductionR G angleG km kg kt ktm nug num nugt "
        "mu mum mumb murf distVerlet dtt iterDEM freq amp t").split()] + [
        ("updateVerlet", C.c_int), ("stepFilm", C.c_int)]


class Config(C.Structure):
    """lbmdem_config"""
    _fields_ = [("lx", C.c_int), ("ly", C.c_int), ("x_begin", C.c_int), ("x_end", C.c_int),
                ("halo", C.c_int), ("device", C.c_int), ("nbgrains", C.c_int), ("scale", C.c_double),
                ("dx", C.c_double), ("dtLB", C.c_double), ("c", C.c_double), ("dt", C.c_double),
                ("dt2", C.c_double), ("npDEM", C.c_int),
                ("Mgx", C.c_double), ("Mdx", C.c_double), ("Mby", C.c_double), ("Mhy", C.c_double),
                ("xG", C.c_double), ("yG", C.c_double), ("phys", Physics)]


class SceneEvent(C.Structure):
    """lbmdem_scene_event"""
    _fields_ = [("kind", C.c_int), ("nfile", C.c_int), ("step", C.c_long)]


_SAY = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)


class Scene(C.Structure):
    """lbmdem_scene"""
    _fields_ = [("dir", C.c_char_p), ("fluid", C.c_int), ("duration", C.c_double), ("say", _SAY), ("user", C.c_void_p)]


class SceneResult(C.Structure):
    """lbmdem_scene_result"""
    _fields_ = [("steps_done", C.c_long), ("nfile", C.c_int), ("stopped", C.c_int), ("energies8", C.c_double * 8),
                ("last_density", C.c_double)]


class ProbeConfig(C.Structure):
    """lbmdem_probe_config"""
    _fields_ = [("every", C.c_int), ("capacity", C.c_int), ("pressure_row", C.c_int), ("velocity_row", C.c_int),
                ("npoints", C.c_int), ("points", C.POINTER(C.c_int)), ("grain_extent", C.c_int)]


SCENE_KINDS = ("CONSOLE_DENSITY", "VTK", "DEM", "STEPS_LINE", "STOP")

_lib = None
_lib_sp = None
SP_LIB_PATH = os.path.join(_HERE, "liblbmdem_hip_sp.so")   # `real` = float: the reference's -DSINGLE_PRECISION mode


def load_library(precision="f64"):
    """dlopen liblbmdem_hip.so (precision "f32": liblbmdem_hip_sp.so, same ABI); fails loudly when it has not been built."""
    global _lib, _lib_sp
    if precision == "f32":
        if _lib_sp is None:
            load_library()       # runtime set-up (torch first, kernel arguments) happens with the default library
            _lib_sp = _open_library(SP_LIB_PATH)
        return _lib_sp
    if _lib is not None:
        return _lib
    _lib = _open_library(LIB_PATH)
    return _lib


def _open_library(LIB_PATH):
    if not os.path.exists(LIB_PATH):
        raise LbmDemError(-2, f"{LIB_PATH} not built -- run __graft_entry__.build() "
                              "(make -C 2d-lbm-dem_amd/csrc); there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (requested by the
    # unversioned name), liblbmdem_hip.so links the system one (libamdhip64.so.7). If ours were
    # loaded first and torch later (the strip driver uses torch.distributed), the process would end
    # up with two runtimes and torch would see no GPU. Importing torch first makes both share one.
    # Launch latency: the HIP runtime places kernel arguments in host memory by default on this stack; a step
    # is ~17 dependent launches, 12 of them ~8 us DEM sub-steps, and device-resident arguments
    # (HIP_FORCE_DEV_KERNARG, read when the runtime initialises) take ~1.2 us off each (measured: 1.182 ->
    # 1.163 ms per coupled step). Only a default: an explicit setting of the caller wins.
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.lbmdem_last_error.restype = C.c_char_p
    L.lbmdem_version.restype = C.c_char_p
    L.lbmdem_nbsteps.restype = C.c_long
    L.lbmdem_nbsteps.argtypes = [C.c_void_p]
    L.lbmdem_halo_doubles.restype = C.c_long
    L.lbmdem_halo_doubles.argtypes = [C.c_void_p]
    L.lbmdem_free_host.argtypes = [C.c_void_p]
    L.lbmdem_free_host.restype = None
    L.lbmdem_run.argtypes = [C.c_void_p, C.c_long]
    L.lbmdem_run_dem.argtypes = [C.c_void_p, C.c_long]
    L.lbmdem_set_nbsteps.argtypes = [C.c_void_p, C.c_long]
    L.lbmdem_derive.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]
    L.lbmdem_create.argtypes = [C.POINTER(Config), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    for name in ("destroy", "lbm_step", "obst_construction", "collide_stream", "forces_fluid",
                 "verlet_rebuild", "dem_substep", "sync", "use_own_stream"):
        getattr(L, "lbmdem_" + name).argtypes = [C.c_void_p]
    for name in ("upload_f", "download_f", "download_obst", "total_density", "upload_kinematics",
                 "download_kinematics", "download_fhf", "set_stream"):
        getattr(L, "lbmdem_" + name).argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_path_info.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_fused_work_order.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_dist_export_carries.argtypes = [C.c_void_p] * 4
    L.lbmdem_dist_set_carries.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_dist_export_owned.argtypes = [C.c_void_p] * 5
    L.lbmdem_dist_table_substep.argtypes = [C.c_void_p] * 4
    L.lbmdem_vtk_place_owned.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_write_vtk_fields.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lbmdem_total_density_serial.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    L.lbmdem_download_macro.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_download_verlet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lbmdem_download_grain_pressure.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_download_vtk_fields.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    L.lbmdem_write_vtk.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_set_async_output.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_write_vtk_async.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_output_drain.argtypes = [C.c_void_p]
    L.lbmdem_output_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_vtk_image_bytes.argtypes = [C.c_int, C.c_int]
    L.lbmdem_vtk_image_bytes.restype = C.c_size_t
    L.lbmdem_write_vtk_image.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lbmdem_download_vtk_image.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_dem_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_set_async_dem.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_write_dem_async.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    L.lbmdem_output_stats_dem.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_write_dem_rows.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.lbmdem_set_diagnostics.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_download_grain_table.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_write_dem.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    L.lbmdem_write_forces.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_geometry_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_download_act.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_download_links.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_geometry_obst.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_write_obst.argtypes = [C.c_void_p, C.c_char_p]
    L.lbmdem_write_obst_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.lbmdem_contact_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_download_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_write_contacts.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_set_contacts_output.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_write_contacts_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_long, C.c_int, C.c_int]
    L.lbmdem_cluster_compute.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
    L.lbmdem_download_cluster_grains.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    L.lbmdem_cluster_grains_device.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4
    L.lbmdem_download_clusters.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_cluster_rounds.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_write_clusters.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_int]
    L.lbmdem_set_clusters_output.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int]
    L.lbmdem_write_clusters_files.argtypes = ([C.c_char_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_long] + [C.c_void_p] * 5 +
                                              [C.c_long, C.c_double, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_double, C.c_int,
                                               C.c_int])
    L.lbmdem_structure_edges.argtypes = [C.c_double, C.c_int, C.c_void_p]
    L.lbmdem_structure_compute.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_long, C.c_void_p]
    L.lbmdem_download_structure_grains.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    L.lbmdem_structure_grains_device.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 6
    L.lbmdem_download_structure_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.lbmdem_download_structure_neighbours.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_write_structure.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_double]
    L.lbmdem_set_structure_output.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double]
    L.lbmdem_write_structure_files.argtypes = ([C.c_char_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_double, C.c_int, C.c_double] +
                                               [C.c_void_p] * 2 + [C.c_double] * 3)
    L.lbmdem_voronoi_compute.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_download_voronoi_grains.argtypes = [C.c_void_p] + [C.c_void_p] * 8
    L.lbmdem_voronoi_grains_device.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 8
    L.lbmdem_download_voronoi_faces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_write_voronoi.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_double]
    L.lbmdem_set_voronoi_output.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.lbmdem_write_voronoi_files.argtypes = ([C.c_char_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_double, C.c_void_p] +
                                             [C.c_double] * 3)
    L.lbmdem_strain_mark.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    L.lbmdem_strain_clear.argtypes = [C.c_void_p]
    L.lbmdem_strain_compute.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_download_strain_grains.argtypes = [C.c_void_p] + [C.c_void_p] * 11
    L.lbmdem_strain_grains_device.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 11
    L.lbmdem_download_strain_reference.argtypes = ([C.c_void_p] + [C.c_void_p] * 5 + [C.c_long, C.POINTER(C.c_long),
                                                   C.POINTER(C.c_double), C.POINTER(C.c_long)])
    L.lbmdem_write_strain.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_int]
    L.lbmdem_set_strain_output.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int]
    L.lbmdem_write_strain_files.argtypes = ([C.c_char_p, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_double, C.c_void_p] +
                                            [C.c_double] * 2)
    L.lbmdem_pore_compute.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lbmdem_download_pore_labels.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_pore_labels_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.lbmdem_download_pores.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_pore_grains.argtypes = [C.c_void_p] + [C.c_void_p] * 3
    L.lbmdem_pore_grains_device.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3
    L.lbmdem_write_pores.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.lbmdem_set_pores_output.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.lbmdem_write_pore_files.argtypes = ([C.c_char_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_long, C.c_int] +
                                          [C.c_void_p] * 4 + [C.c_double])
    L.lbmdem_clearance_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    L.lbmdem_download_clearance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_clearance_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.lbmdem_download_clearance_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_clearance_owners.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_clearance_owners_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.lbmdem_download_throats.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_write_clearance.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    L.lbmdem_set_clearance_output.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbmdem_write_clearance_files.argtypes = ([C.c_char_p] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_long, C.c_void_p, C.c_long, C.c_int] +
                                               [C.c_void_p] * 3 + [C.c_double])
    L.lbmdem_network_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p]
    L.lbmdem_download_network.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_network_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.lbmdem_download_network_bodies.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_network_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_network_links.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_write_network.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.lbmdem_set_network_output.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.lbmdem_write_network_files.argtypes = ([C.c_char_p] + [C.c_int] * 6 + [C.c_void_p] * 3 + [C.c_long, C.c_void_p, C.c_long, C.c_void_p,
                                              C.c_long, C.c_void_p, C.c_double])
    L.lbmdem_drainage_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p]
    L.lbmdem_download_drainage.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_drainage_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.lbmdem_download_drainage_bodies.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_drainage_links.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_drainage_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_drainage_rounds.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.lbmdem_write_drainage.argtypes = [C.c_void_p, C.c_char_p] + [C.c_int] * 5
    L.lbmdem_set_drainage_output.argtypes = [C.c_void_p] + [C.c_int] * 5
    L.lbmdem_write_drainage_files.argtypes = ([C.c_char_p] + [C.c_int] * 8 + [C.c_void_p] * 2 + [C.c_long, C.c_void_p, C.c_long, C.c_void_p,
                                               C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_double])
    L.lbmdem_geodesic_compute.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_long, C.c_void_p]
    L.lbmdem_download_geodesic.argtypes = [C.c_void_p] + [C.c_void_p] * 3
    L.lbmdem_geodesic_device.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_int)]
    L.lbmdem_download_geodesic_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_geodesic_rounds.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lbmdem_write_geodesic.argtypes = [C.c_void_p, C.c_char_p] + [C.c_int] * 7
    L.lbmdem_set_geodesic_output.argtypes = [C.c_void_p] + [C.c_int] * 7
    L.lbmdem_write_geodesic_files.argtypes = ([C.c_char_p] + [C.c_int] * 10 + [C.c_void_p] * 4 + [C.c_long, C.c_void_p, C.c_double])
    L.lbmdem_netflux_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.lbmdem_download_netflux_links.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_netflux_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_netflux_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_write_netflux.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.lbmdem_set_netflux_output.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.lbmdem_write_netflux_files.argtypes = ([C.c_char_p] + [C.c_int] * 6 + [C.c_void_p] * 2 + [C.c_long] + [C.c_void_p] * 3 + [C.c_long] +
                                             [C.c_void_p] * 3 + [C.c_double])
    L.lbmdem_netsolve_compute.argtypes = ([C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_double, C.c_int, C.c_void_p,
                                                                                  C.c_void_p])
    L.lbmdem_download_netsolve_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_download_netsolve_links.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_netsolve_rounds.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.lbmdem_write_netsolve.argtypes = [C.c_void_p, C.c_char_p] + [C.c_int] * 6 + [C.c_double, C.c_int]
    L.lbmdem_set_netsolve_output.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_double, C.c_int]
    L.lbmdem_write_netsolve_files.argtypes = ([C.c_char_p] + [C.c_int] * 9 + [C.c_void_p, C.c_long] * 4 + [C.c_void_p, C.c_void_p,
                                                                                                            C.c_double])
    L.lbmdem_coarse_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lbmdem_coarse_fields.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.c_void_p]
    L.lbmdem_write_coarse.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.lbmdem_write_coarse_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int]
    L.lbmdem_set_coarse_output.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbmdem_flow_fields.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_flow_fields_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    L.lbmdem_flow_sums.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_write_flow.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_write_flow_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    L.lbmdem_set_flow_output.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_tracer_set.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_int]
    L.lbmdem_tracer_advance.argtypes = [C.c_void_p]
    L.lbmdem_tracer_download.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_tracer_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.lbmdem_tracer_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_tracer_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_write_tracers.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_write_tracers_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_void_p]
    L.lbmdem_set_tracer_output.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_scalar_set.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int]
    L.lbmdem_scalar_step.argtypes = [C.c_void_p]
    L.lbmdem_scalar_download.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_scalar_download_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_scalar_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int]
    L.lbmdem_scalar_sums.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_scalar_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_write_scalar.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_write_scalar_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lbmdem_set_scalar_output.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_mean_begin.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for name in ("mean_sample", "mean_reset", "mean_end"):
        getattr(L, "lbmdem_" + name).argtypes = [C.c_void_p]
    L.lbmdem_mean_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_mean_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_mean_fields.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_mean_fields_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    L.lbmdem_mean_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.lbmdem_write_mean.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_write_mean_files.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_long] + [C.c_void_p] * 8
    L.lbmdem_set_mean_output.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.lbmdem_write_densities.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.lbmdem_download_densities_text.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lbmdem_set_densities_staging.argtypes = [C.c_void_p, C.c_size_t]
    L.lbmdem_densities_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_write_densities_host.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.lbmdem_format_fixed4.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    L.lbmdem_collide_stream_part.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_checkpoint_save.argtypes = [C.c_void_p, C.c_char_p]
    L.lbmdem_checkpoint_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    L.lbmdem_set_async_checkpoint.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_checkpoint_save_async.argtypes = [C.c_void_p, C.c_char_p]
    L.lbmdem_output_stats_checkpoint.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_set_checkpoint_every.argtypes = [C.c_void_p, C.c_long, C.c_char_p]
    L.lbmdem_checkpoint_digest.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.lbmdem_checkpoint_verify.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.lbmdem_set_checkpoint_contents.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_checkpoint_contents.argtypes = [C.c_char_p, C.c_void_p]
    L.lbmdem_set_force_mode.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_set_dem_chain.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_dem_chain_paints.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    if hasattr(L, "lbmdem_set_dem_tiles"):
        L.lbmdem_set_dem_tiles.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "lbmdem_dem_chain_recoveries"):   # (older builds kept for A/B runs do not have it)
        L.lbmdem_dem_chain_recoveries.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
    if hasattr(L, "lbmdem_debug_chain_giveup"):   # experiment build only
        L.lbmdem_debug_chain_giveup.argtypes = [C.c_void_p, C.c_int]
        L.lbmdem_debug_live_memory.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.lbmdem_set_obst_update.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_obst_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.lbmdem_set_change_mask.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_change_mask_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.lbmdem_measure_copy.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    L.lbmdem_dem_chain_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lbmdem_set_lid.argtypes = [C.c_void_p, C.c_double]
    L.lbmdem_set_vibration.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_vibration.argtypes = [C.c_void_p]
    L.lbmdem_move_walls.argtypes = [C.c_void_p]
    L.lbmdem_get_walls.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_vibration_schedule.argtypes = [C.POINTER(Config), C.c_long, C.c_long, C.c_void_p]
    L.lbmdem_scene_schedule.argtypes = [C.POINTER(Config), C.c_long, C.c_long, C.c_double, C.c_int, C.c_void_p, C.c_long,
                                        C.POINTER(C.c_long)]
    L.lbmdem_run_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(Scene), C.POINTER(SceneResult)]
    L.lbmdem_probe_enable.argtypes = [C.c_void_p, C.POINTER(ProbeConfig)]
    L.lbmdem_probe_disable.argtypes = [C.c_void_p]
    L.lbmdem_probe_record_doubles.argtypes = [C.c_void_p]
    L.lbmdem_probe_record_doubles.restype = C.c_long
    L.lbmdem_probe_layout.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_probe_read.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.lbmdem_force_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lbmdem_profile_enable.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_halo_pack.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.lbmdem_halo_unpack.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.lbmdem_dist_default_margin.argtypes = [C.c_void_p]
    L.lbmdem_dist_enable.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_dist_message_doubles.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_dist_message_doubles.restype = C.c_long
    L.lbmdem_dist_begin_period.argtypes = [C.c_void_p]
    L.lbmdem_dist_pack.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.lbmdem_dist_unpack.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.lbmdem_dist_set_poison.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_dist_pack2.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lbmdem_dist_unpack2.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.lbmdem_halo_pack2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_halo_unpack2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.lbmdem_comm_unique_id.argtypes = [C.c_void_p]
    L.lbmdem_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.lbmdem_comm_destroy.argtypes = [C.c_void_p]
    L.lbmdem_comm_lbm_step.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_comm_run.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    L.lbmdem_comm_allreduce_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.lbmdem_comm_selftest.argtypes = [C.c_void_p, C.c_int]
    L.lbmdem_fhf_export.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_fhf_import.argtypes = [C.c_void_p, C.c_void_p]
    L.lbmdem_fhf_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.lbmdem_get_config.argtypes = [C.c_void_p, C.POINTER(Config)]
    L.lbmdem_read_sample.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_double)),
                                     C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_double))]
    return L


def live_memory():
    """(blocks, bytes) of device and pinned memory the library holds in this process right now. Experiment build only."""
    L = load_library()
    if not hasattr(L, "lbmdem_debug_live_memory"):
        raise LbmDemError(-1, "live_memory: only the experiment build (make AB=1) counts its memory")
    blocks, nbytes = C.c_long(0), C.c_long(0)
    _chk(L.lbmdem_debug_live_memory(C.byref(blocks), C.byref(nbytes)))
    return int(blocks.value), int(nbytes.value)


def strips_module():
    """The x-strip decomposition driver (one process per GPU), imported lazily."""
    from . import strips
    return strips


def write_vtk_fields(directory, nFile, lx, ly, fields11):
    """the five VTK files of write_vtk (main.c:237-338) from merged lattice-sized fields (LbmDem.vtk_place_owned)"""
    f = np.ascontiguousarray(fields11, dtype=np.float32)
    _chk(load_library().lbmdem_write_vtk_fields(os.fsencode(directory), int(nFile), int(lx), int(ly), _vp(f)))


def vtk_image_bytes(lx, ly):
    """size of a frame image: the five VTK payloads as the files hold them, back to back (44 bytes per node)"""
    return int(load_library().lbmdem_vtk_image_bytes(int(lx), int(ly)))


def write_vtk_image(directory, nFile, lx, ly, image):
    """the five VTK files of write_vtk from a frame image (LbmDem.vtk_image): big-endian float32, grain_pressure[ly][lx],
    grain_velocity[ly][lx][3], grain_acceleration[ly][lx][3], fluid_pressure[ly][lx], fluid_velocity[ly][lx][3]. Host only."""
    buf = np.frombuffer(image, dtype=np.uint8) if not isinstance(image, np.ndarray) else np.ascontiguousarray(image).view(np.uint8).reshape(-1)
    if buf.size != 44 * max(int(lx), 0) * max(int(ly), 0):
        raise LbmDemError(-1, f"write_vtk_image: the image of a {lx} x {ly} lattice has {44 * int(lx) * int(ly)} bytes, not {buf.size}")
    _chk(load_library().lbmdem_write_vtk_image(os.fsencode(directory), int(nFile), int(lx), int(ly), _vp(buf)))


# struct lbmdem_link: an effective boundary link (LbmDem.download_links); q < 0 flags a delta of exactly zero
LINK_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("q", np.int32), ("grain", np.int32), ("delta", np.float64)])
GEOMETRY_COUNTERS = ("solid_nodes", "active_nodes", "links", "links_near", "links_far", "solid_slots")


def write_obst_files(directory, obst, act, links):
    """obst_writing (main.c:1601-1641): obst_LB.dat, active_nodes.dat and links.dat from the two [lx][ly] maps and a link list
    (LINK_DTYPE, the file's order). Host only."""
    obst = np.ascontiguousarray(obst, dtype=np.int32)
    act = np.ascontiguousarray(act, dtype=np.int32)
    links = np.ascontiguousarray(links, dtype=LINK_DTYPE)
    if obst.ndim != 2 or act.shape != obst.shape or links.ndim != 1:
        raise LbmDemError(-1, "write_obst_files: obst and act must be [lx][ly] maps of one shape, links a list of LINK_DTYPE")
    _chk(load_library().lbmdem_write_obst_files(os.fsencode(directory), obst.shape[0], obst.shape[1], _vp(obst), _vp(act),
                                                _vp(links), len(links)))


# struct lbmdem_contact: a contact of the last table sub-step (LbmDem.download_contacts); j < 0 is a wall code
WALL_B, WALL_T, WALL_L, WALL_R = -1, -2, -3, -4


class Contact(C.Structure):
    """lbmdem_contact"""
    _fields_ = [("i", C.c_int), ("j", C.c_int), ("dn", C.c_double), ("nx", C.c_double), ("ny", C.c_double),
                ("fn", C.c_double), ("ft", C.c_double)]


CONTACT_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("dn", np.float64), ("nx", np.float64), ("ny", np.float64),
                          ("fn", np.float64), ("ft", np.float64)])
CONTACT_COUNTERS = ("candidate_pairs", "touching_pairs", "coulomb_clamped", "fn_zero", "wall_contacts", "grains_in_contact")


def write_contacts_files(directory, nFile, r, x1, x2, fm, contacts, lx, ly, precision="f64"):
    """contacts%.6i.dat ("# i j dn nx ny fn ft", then one "%d %d %le %le %le %le %le" line per record) and DEM%.6i_chains.ps (the
    discs of write_forces, then every grain-grain record with fn > 0 as a line of width fn) from per-grain r, x1, x2, fm and a
    record list (CONTACT_DTYPE). Host only."""
    cols = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (r, x1, x2, fm)]
    rec = np.ascontiguousarray(contacts, dtype=CONTACT_DTYPE).reshape(-1)
    n = len(cols[0])
    if any(len(a) != n for a in cols):
        raise LbmDemError(-1, "write_contacts_files: r, x1, x2 and fm must have one value per grain")
    _chk(load_library(precision).lbmdem_write_contacts_files(os.fsencode(directory), int(nFile), n, _vp(cols[0]), _vp(cols[1]),
                                                             _vp(cols[2]), _vp(cols[3]), _vp(rec) if len(rec) else None,
                                                             len(rec), int(lx), int(ly)))


# struct lbmdem_cluster: one component of two or more grains of the contact net (LbmDem.cluster_table), 56 bytes
CLUSTER_DTYPE = np.dtype([("label", np.int32), ("size", np.int32), ("contacts", np.int64), ("walls", np.int32), ("core", np.int32),
                          ("xmin", np.float64), ("xmax", np.float64), ("ymin", np.float64), ("ymax", np.float64)])
CLUSTER_COUNTERS = ("selected_pairs", "selected_walls", "clusters", "largest_size", "largest_label", "isolated_grains",
                    "core_grains", "core_pairs", "core_walls", "spanning")


def write_clusters_files(directory, nFile, r, x1, x2, fm, contacts, label, degree, core, walls, table, fmin, relative, zmin, thr,
                         counts, t, lx, ly, precision="f64"):
    """clusters%.6i.dat, cluster_table%.6i.dat, DEM%.6i_clusters.ps and one appended line of clusters.data (include/lbmdem_hip.h
    spells the four formats out) from per-grain r, x1, x2, fm, a record list (CONTACT_DTYPE), the four per-grain results, the
    table (CLUSTER_DTYPE), the three parameters, the threshold, the ten counts (a dict of CLUSTER_COUNTERS or a sequence) and
    the time of the line. Host only."""
    cols = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (r, x1, x2, fm)]
    ints = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (label, degree, core, walls)]
    rec = np.ascontiguousarray(contacts, dtype=CONTACT_DTYPE).reshape(-1)
    tab = np.ascontiguousarray(table, dtype=CLUSTER_DTYPE).reshape(-1)
    if isinstance(counts, dict):
        counts = [counts[k] for k in CLUSTER_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    n = len(cols[0])
    if any(len(a) != n for a in cols + ints) or len(cnt) != len(CLUSTER_COUNTERS):
        raise LbmDemError(-1, "write_clusters_files: r, x1, x2, fm, label, degree, core and walls must have one value per grain, "
                              "counts ten")
    _chk(load_library(precision).lbmdem_write_clusters_files(
        os.fsencode(directory), int(nFile), n, *(_vp(a) for a in cols), _vp(rec) if len(rec) else None, len(rec),
        *(_vp(a) for a in ints), _vp(tab) if len(tab) else None, len(tab), float(fmin), int(bool(relative)), int(zmin), float(thr),
        _vp(cnt), float(t), int(lx), int(ly)))


# the per-grain results of LbmDem.structure() (LbmDem.structure_grains), and the names of its eight counts
STRUCTURE_DTYPE = np.dtype([("nb", np.int32), ("bonds", np.int32), ("c6", np.float64), ("s6", np.float64), ("c2", np.float64),
                            ("s2", np.float64)])
STRUCTURE_COUNTERS = ("entries", "pairs", "bonded_pairs", "max_neighbours", "lone_grains", "six_bonds", "coincident_pairs",
                      "nonfinite_grains")


def structure_edges(rcut, nbins, precision="f64"):
    """the squared bin edges of the pair histogram, e2[nbins + 1] (include/lbmdem_hip.h: the table alone decides a bin). Host only."""
    e2 = np.zeros(max(int(nbins), 0) + 1, np.float64)
    _chk(load_library(precision).lbmdem_structure_edges(float(rcut), int(nbins), _vp(e2)))
    return e2


def write_structure_files(directory, nFile, grains, rcut, nbins, shell, hist, counts, t, W, H, precision="f64"):
    """structure%.6i.dat, gr%.6i.dat and one appended line of structure.data (include/lbmdem_hip.h spells the three formats out) from
    the per-grain results (STRUCTURE_DTYPE), the parameters, the histogram, the eight counts (a dict of STRUCTURE_COUNTERS or a
    sequence), the time of the line and the box's extent. Host only."""
    g = np.ascontiguousarray(grains, dtype=STRUCTURE_DTYPE).reshape(-1)
    ints = [np.ascontiguousarray(g[k]) for k in ("nb", "bonds")]
    dbl = [np.ascontiguousarray(g[k]) for k in ("c6", "s6", "c2", "s2")]
    if isinstance(counts, dict):
        counts = [counts[k] for k in STRUCTURE_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    hh = np.ascontiguousarray(hist, dtype=np.int64).reshape(-1)
    if len(cnt) != len(STRUCTURE_COUNTERS) or len(hh) != int(nbins):
        raise LbmDemError(-1, "write_structure_files: counts must have eight values, hist one per bin")
    _chk(load_library(precision).lbmdem_write_structure_files(
        os.fsencode(directory), int(nFile), len(g), *(_vp(a) for a in ints), *(_vp(a) for a in dbl), float(rcut), int(nbins),
        float(shell), _vp(hh), _vp(cnt), float(t), float(W), float(H)))


# the per-grain results of LbmDem.voronoi() (LbmDem.voronoi_grains), the names of its eight counts, and the bits of `flags`
VORONOI_DTYPE = np.dtype([("area", np.float64), ("perimeter", np.float64), ("phi", np.float64), ("R2", np.float64),
                          ("faces", np.int32), ("walls", np.int32), ("nverts", np.int32), ("flags", np.int32)])
VORONOI_COUNTERS = ("cells", "complete", "empty", "overflowed", "nonfinite_grains", "grain_faces", "wall_faces", "max_faces")
VOR_MAXV = 32
VOR_COMPLETE, VOR_EMPTY, VOR_OVERFLOW, VOR_NONFINITE = 1, 2, 4, 8


def write_voronoi_files(directory, nFile, grains, rcut, counts, t, W, H, precision="f64"):
    """voronoi%.6i.dat and one appended line of voronoi.data (include/lbmdem_hip.h spells the two formats out) from the per-grain
    results (VORONOI_DTYPE), the cutoff, the eight counts (a dict of VORONOI_COUNTERS or a sequence), the time of the line and the
    box's extent. Host only."""
    g = np.ascontiguousarray(grains, dtype=VORONOI_DTYPE).reshape(-1)
    cols = [np.ascontiguousarray(g[k]) for k in ("area", "perimeter", "phi", "faces", "walls", "nverts", "flags")]
    if isinstance(counts, dict):
        counts = [counts[k] for k in VORONOI_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(cnt) != len(VORONOI_COUNTERS):
        raise LbmDemError(-1, "write_voronoi_files: counts must have eight values")
    _chk(load_library(precision).lbmdem_write_voronoi_files(
        os.fsencode(directory), int(nFile), len(g), *(_vp(a) for a in cols), float(rcut), _vp(cnt), float(t), float(W), float(H)))


# the per-grain results of LbmDem.strain() (LbmDem.strain_grains), the names of its eight counts, and the bits of `flags`
STRAIN_DTYPE = np.dtype([("ux", np.float64), ("uy", np.float64), ("drot", np.float64), ("Fxx", np.float64), ("Fxy", np.float64),
                         ("Fyx", np.float64), ("Fyy", np.float64), ("d2min", np.float64), ("used", np.int32), ("lost", np.int32),
                         ("flags", np.int32)])
STRAIN_COUNTERS = ("fitted", "few", "degenerate", "nonfinite_grains", "entries", "used", "lost", "worst_grain")
STRAIN_NONFINITE, STRAIN_FEW, STRAIN_DEGENERATE = 1, 2, 4


def write_strain_files(directory, nFile, grains, rc2, counts, t, t_mark, precision="f64"):
    """strain%.6i.dat and one appended line of strain.data (include/lbmdem_hip.h spells the two formats out) from the per-grain
    results (STRAIN_DTYPE), the square of the mark's cutoff, the eight counts (a dict of STRAIN_COUNTERS or a sequence), the time
    of the line and the time of the mark. Host only."""
    g = np.ascontiguousarray(grains, dtype=STRAIN_DTYPE).reshape(-1)
    cols = [np.ascontiguousarray(g[k]) for k in STRAIN_DTYPE.names]
    if isinstance(counts, dict):
        counts = [counts[k] for k in STRAIN_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(cnt) != len(STRAIN_COUNTERS):
        raise LbmDemError(-1, "write_strain_files: counts must have eight values")
    _chk(load_library(precision).lbmdem_write_strain_files(
        os.fsencode(directory), int(nFile), len(g), *(_vp(a) for a in cols), float(rc2), _vp(cnt), float(t), float(t_mark)))


# struct lbmdem_pore: one connected component of the fluid phase (LbmDem.pore_table), 56 bytes; the names of the ten counts of
# LbmDem.pores()
PORE_DTYPE = np.dtype([("label", np.int32), ("walls", np.int32), ("nodes", np.int64), ("grain_links", np.int64),
                       ("wall_links", np.int64), ("mass_q32", np.int64), ("xmin", np.int32), ("xmax", np.int32), ("ymin", np.int32),
                       ("ymax", np.int32)])
PORE_COUNTERS = ("fluid_nodes", "components", "largest_nodes", "largest_label", "trapped_nodes", "single_nodes", "spanning",
                 "throat_grains", "dry_grains", "unaccumulated")


def write_pore_files(directory, nFile, conn, lx, ly, table, wet, pore_min, pore_max, counts, t, label=None, precision="f64"):
    """pore_table%.6i.dat, pore_grains%.6i.dat, one appended line of pores.data and, with a label plane (lx, ly),
    pores%.6i.vtk (include/lbmdem_hip.h spells the four formats out) from the table (PORE_DTYPE), the three per-grain results,
    the ten counts (a dict of PORE_COUNTERS or a sequence) and the time of the line. Host only."""
    tab = np.ascontiguousarray(table, dtype=PORE_DTYPE).reshape(-1)
    ints = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (wet, pore_min, pore_max)]
    if isinstance(counts, dict):
        counts = [counts[k] for k in PORE_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    n = len(ints[0])
    if any(len(a) != n for a in ints) or len(cnt) != len(PORE_COUNTERS):
        raise LbmDemError(-1, "write_pore_files: wet, pore_min and pore_max must have one value per grain, counts ten")
    lab = None
    if label is not None:
        lab = np.ascontiguousarray(label, dtype=np.int32)
        if lab.shape != (int(lx), int(ly)):
            raise LbmDemError(-1, "write_pore_files: a label plane of shape (lx, ly)")
    _chk(load_library(precision).lbmdem_write_pore_files(
        os.fsencode(directory), int(nFile), int(conn), int(lx), int(ly), 0 if lab is None else 1, None if lab is None else _vp(lab),
        _vp(tab) if len(tab) else None, len(tab), n, *(_vp(a) for a in ints), _vp(cnt), float(t)))


# struct lbmdem_throat: the ridge between the regions of two owners (LbmDem.throat_table), 20 bytes; the names of the ten counts
# of LbmDem.clearance()
THROAT_DTYPE = np.dtype([("lo", np.int32), ("hi", np.int32), ("edges", np.int32), ("c_min", np.int32), ("node", np.int32)])
CLEARANCE_COUNTERS = ("fluid_nodes", "d2_max", "d2_max_node", "sum_d2", "ridge_edges", "throats", "grain_throats", "narrowest_c",
                      "ownerless_grains", "kmax")


def write_clearance_files(directory, nFile, lx, ly, table, hist, owned, d2max, counts, t, d2=None, owner=None, precision="f64"):
    """throats%.6i.dat, clearance_hist%.6i.dat, clearance_owners%.6i.dat, one appended line of clearance.data and, with the two
    planes (lx, ly), clearance%.6i.vtk (include/lbmdem_hip.h spells the five formats out) from the throat table (THROAT_DTYPE),
    the histogram, the two per-owner results [n + 1], the ten counts (a dict of CLEARANCE_COUNTERS or a sequence) and the time
    of the line. Host only."""
    tab = np.ascontiguousarray(table, dtype=THROAT_DTYPE).reshape(-1)
    hs = np.ascontiguousarray(hist, dtype=np.int64).reshape(-1)
    ow = np.ascontiguousarray(owned, dtype=np.int64).reshape(-1)
    dm = np.ascontiguousarray(d2max, dtype=np.int32).reshape(-1)
    if isinstance(counts, dict):
        counts = [counts[k] for k in CLEARANCE_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(ow) != len(dm) or len(ow) < 2 or len(cnt) != len(CLEARANCE_COUNTERS):
        raise LbmDemError(-1, "write_clearance_files: owned and d2max must have one value per grain and one for the wall, counts ten")
    if (d2 is None) != (owner is None):
        raise LbmDemError(-1, "write_clearance_files: d2 and owner come together")
    planes = None
    if d2 is not None:
        planes = [np.ascontiguousarray(a, dtype=np.int32) for a in (d2, owner)]
        if any(a.shape != (int(lx), int(ly)) for a in planes):
            raise LbmDemError(-1, "write_clearance_files: planes of shape (lx, ly)")
    _chk(load_library(precision).lbmdem_write_clearance_files(
        os.fsencode(directory), int(nFile), int(lx), int(ly), 0 if planes is None else 1, None if planes is None else _vp(planes[0]),
        None if planes is None else _vp(planes[1]), _vp(tab) if len(tab) else None, len(tab), _vp(hs) if len(hs) else None, len(hs),
        len(ow) - 1, _vp(ow), _vp(dm), _vp(cnt), float(t)))


# struct lbmdem_net_body, lbmdem_net_link, lbmdem_net_group: the records of the pore network (LbmDem.network_bodies,
# network_links, network_groups), 32, 20 and 32 bytes; the names of the ten counts of LbmDem.network()
NET_BODY_DTYPE = np.dtype([("node", np.int32), ("d2", np.int32), ("nodes", np.int64), ("degree", np.int32), ("parent", np.int32),
                           ("group", np.int32)], align=True)
NET_LINK_DTYPE = np.dtype([("lo", np.int32), ("hi", np.int32), ("edges", np.int32), ("saddle", np.int32), ("node", np.int32)])
NET_GROUP_DTYPE = np.dtype([("body", np.int32), ("bodies", np.int32), ("nodes", np.int64), ("d2", np.int32), ("node", np.int32),
                            ("degree", np.int32)], align=True)
NETWORK_COUNTERS = ("fluid_nodes", "bodies", "body_links", "body_edges", "groups", "group_links", "group_edges", "isolated_groups",
                    "largest_group_nodes", "narrowest_saddle")


def write_network_files(directory, nFile, lx, ly, n, merge, bodies, groups, links, counts, t, body=None, group=None, precision="f64"):
    """network_bodies%.6i.dat, network_links%.6i.dat, network_groups%.6i.dat, one appended line of network.data and, with the two
    planes (lx, ly), network%.6i.vtk (include/lbmdem_hip.h spells the five formats out) from the body table (NET_BODY_DTYPE), the
    group table (NET_GROUP_DTYPE), the links between the groups (NET_LINK_DTYPE), the ten counts (a dict of NETWORK_COUNTERS or a
    sequence) and the time of the line; n: the grain count of the first lines. Host only."""
    bo = np.ascontiguousarray(bodies, dtype=NET_BODY_DTYPE).reshape(-1)
    gr = np.ascontiguousarray(groups, dtype=NET_GROUP_DTYPE).reshape(-1)
    li = np.ascontiguousarray(links, dtype=NET_LINK_DTYPE).reshape(-1)
    if isinstance(counts, dict):
        counts = [counts[k] for k in NETWORK_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(cnt) != len(NETWORK_COUNTERS):
        raise LbmDemError(-1, "write_network_files: ten counts")
    if (body is None) != (group is None):
        raise LbmDemError(-1, "write_network_files: body and group come together")
    planes = None
    if body is not None:
        planes = [np.ascontiguousarray(a, dtype=np.int32) for a in (body, group)]
        if any(a.shape != (int(lx), int(ly)) for a in planes):
            raise LbmDemError(-1, "write_network_files: planes of shape (lx, ly)")
    _chk(load_library(precision).lbmdem_write_network_files(
        os.fsencode(directory), int(nFile), int(lx), int(ly), int(n), int(merge), 0 if planes is None else 1,
        None if planes is None else _vp(planes[0]), None if planes is None else _vp(planes[1]), _vp(bo) if len(bo) else None, len(bo),
        _vp(gr) if len(gr) else None, len(gr), _vp(li) if len(li) else None, len(li), _vp(cnt), float(t)))


# drainage (LbmDem.drainage): the sides of `frm` and `to`, to be or-ed, and the names of the ten counts
SIDE_B, SIDE_T, SIDE_L, SIDE_R = 1, 2, 4, 8
DRAINAGE_COUNTERS = ("fluid_nodes", "inlet_nodes", "reached_nodes", "reached_bodies", "access_max", "shielded_nodes", "outlet_nodes",
                     "critical", "critical_node", "front_links")


def write_drainage_files(directory, nFile, lx, ly, n, frm, band, to, bodies, A, hist, clearance_hist, counts, t, access=None,
                         precision="f64"):
    """drainage_curve%.6i.dat, drainage_bodies%.6i.dat, one appended line of drainage.data and, with the plane access (lx, ly),
    drainage%.6i.vtk (include/lbmdem_hip.h spells the four formats out) from the network's body table (NET_BODY_DTYPE), A per body,
    the access and the clearance histogram, the ten counts (a dict of DRAINAGE_COUNTERS or a sequence) and the time of the line;
    n: the grain count of the first lines. Host only."""
    bo = np.ascontiguousarray(bodies, dtype=NET_BODY_DTYPE).reshape(-1)
    aa = np.ascontiguousarray(A, dtype=np.int32).reshape(-1)
    hs = np.ascontiguousarray(hist, dtype=np.int64).reshape(-1)
    ch = np.ascontiguousarray(clearance_hist, dtype=np.int64).reshape(-1)
    if isinstance(counts, dict):
        counts = [counts[k] for k in DRAINAGE_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(cnt) != len(DRAINAGE_COUNTERS):
        raise LbmDemError(-1, "write_drainage_files: ten counts")
    plane = None
    if access is not None:
        plane = np.ascontiguousarray(access, dtype=np.int32)
        if plane.shape != (int(lx), int(ly)):
            raise LbmDemError(-1, "write_drainage_files: a plane of shape (lx, ly)")
    _chk(load_library(precision).lbmdem_write_drainage_files(
        os.fsencode(directory), int(nFile), int(lx), int(ly), int(n), int(frm), int(band), int(to), 0 if plane is None else 1,
        None if plane is None else _vp(plane), _vp(bo) if len(bo) else None, len(bo), _vp(aa) if len(aa) else None, len(aa),
        _vp(hs) if len(hs) else None, len(hs), _vp(ch) if len(ch) else None, len(ch), _vp(cnt), float(t)))


# geodesic (LbmDem.geodesic): the names of the ten counts, struct lbmdem_geo_level (one depth of the profile) and the cost of an
# axis step (a diagonal one costs 7)
GEODESIC_COUNTERS = ("fluid_nodes", "passable_nodes", "inlet_nodes", "reached_nodes", "dist_max", "outlet_nodes", "outlet_reached",
                     "shortest", "shortest_node", "path_nodes")
GEO_LEVEL_DTYPE = np.dtype([("nodes", np.int64), ("reached", np.int64), ("sum", np.int64), ("dmin", np.int32), ("dmax", np.int32)])
GEO_UNIT = 5


def write_geodesic_files(directory, nFile, lx, ly, n, frm, band, to, conn, min_d2, levels, counts, t, planes=None, precision="f64"):
    """geodesic_profile%.6i.dat, one appended line of geodesic.data and, with planes = (dist, back, detour), each (lx, ly),
    geodesic%.6i.vtk (include/lbmdem_hip.h spells the three formats out) from the profile (GEO_LEVEL_DTYPE), the ten counts (a
    dict of GEODESIC_COUNTERS or a sequence) and the time of the line; n: the grain count of the first line. Host only."""
    lv = np.ascontiguousarray(levels, dtype=GEO_LEVEL_DTYPE).reshape(-1)
    if isinstance(counts, dict):
        counts = [counts[k] for k in GEODESIC_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(cnt) != len(GEODESIC_COUNTERS):
        raise LbmDemError(-1, "write_geodesic_files: ten counts")
    pl = None
    if planes is not None:
        pl = [np.ascontiguousarray(a, dtype=np.int32) for a in planes]
        if len(pl) != 3 or any(a.shape != (int(lx), int(ly)) for a in pl):
            raise LbmDemError(-1, "write_geodesic_files: three planes of shape (lx, ly)")
    _chk(load_library(precision).lbmdem_write_geodesic_files(
        os.fsencode(directory), int(nFile), int(lx), int(ly), int(n), int(frm), int(band), int(to), int(conn), int(min_d2),
        0 if pl is None else 1, *([None] * 3 if pl is None else [_vp(a) for a in pl]), _vp(lv) if len(lv) else None, len(lv), _vp(cnt),
        float(t)))


# pore fluxes (LbmDem.netflux): struct lbmdem_netflux_link and lbmdem_netflux_region, 24 bytes each, aligned with network_links(level)
# and with network_bodies() (level 0) or network_groups() (level 1); the names of the ten counts
NETFLUX_LINK_DTYPE = np.dtype([("flux_q32", np.int64), ("exchange_q32", np.int64), ("edges", np.int64)])
NETFLUX_REGION_DTYPE = np.dtype([("mass_q32", np.int64), ("net_q32", np.int64), ("through_q32", np.int64)])
NETFLUX_COUNTERS = ("fluid_nodes", "regions", "links", "edges", "ridge_edges", "unaccumulated_edges", "unaccumulated_nodes",
                    "flowing_links", "strongest_link", "largest_imbalance")


def write_netflux_files(directory, nFile, lx, ly, n, merge, level, links, flux, region_body, region_nodes, regions, col, row, counts, t,
                        precision="f64"):
    """netflux_links%.6i.dat, netflux_regions%.6i.dat, netflux_profile%.6i.dat and one appended line of netflux.data
    (include/lbmdem_hip.h spells the four formats out) from the network's links of the level (NET_LINK_DTYPE) and their fluxes
    (NETFLUX_LINK_DTYPE), per region its (root) body number, its node count and its record (NETFLUX_REGION_DTYPE), the two
    profiles (lx - 1 and ly - 1 values), the ten counts (a dict of NETFLUX_COUNTERS or a sequence) and the time of the line;
    n: the grain count of the first lines. Host only."""
    li = np.ascontiguousarray(links, dtype=NET_LINK_DTYPE).reshape(-1)
    fx = np.ascontiguousarray(flux, dtype=NETFLUX_LINK_DTYPE).reshape(-1)
    rb = np.ascontiguousarray(region_body, dtype=np.int32).reshape(-1)
    rn = np.ascontiguousarray(region_nodes, dtype=np.int64).reshape(-1)
    rg = np.ascontiguousarray(regions, dtype=NETFLUX_REGION_DTYPE).reshape(-1)
    co = np.ascontiguousarray(col, dtype=np.int64).reshape(-1)
    ro = np.ascontiguousarray(row, dtype=np.int64).reshape(-1)
    if isinstance(counts, dict):
        counts = [counts[k] for k in NETFLUX_COUNTERS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(cnt) != len(NETFLUX_COUNTERS):
        raise LbmDemError(-1, "write_netflux_files: ten counts")
    if len(li) != len(fx) or len(rb) != len(rg) or len(rn) != len(rg):
        raise LbmDemError(-1, "write_netflux_files: one flux record per link, one body number and one node count per region")
    if len(co) != max(int(lx) - 1, 0) or len(ro) != max(int(ly) - 1, 0):
        raise LbmDemError(-1, "write_netflux_files: col has lx - 1 values and row ly - 1")
    co, ro = (a if len(a) else np.zeros(1, np.int64) for a in (co, ro))
    _chk(load_library(precision).lbmdem_write_netflux_files(
        os.fsencode(directory), int(nFile), int(lx), int(ly), int(n), int(merge), int(level), _vp(li) if len(li) else None,
        _vp(fx) if len(fx) else None, len(li), _vp(rb) if len(rb) else None, _vp(rn) if len(rn) else None,
        _vp(rg) if len(rg) else None, len(rg), _vp(co), _vp(ro), _vp(cnt), float(t)))


# network pressures (LbmDem.netsolve): struct lbmdem_netsolve_region (24 bytes) and lbmdem_netsolve_link (16), aligned with
# network_bodies() (level 0) or network_groups() (level 1) and with network_links(level); the flag bits; the names of the ten counts
# and of the four sums
NETSOLVE_REGION_DTYPE = np.dtype([("p", np.float64), ("net", np.float64), ("flags", np.int32), ("degree", np.int32)])
NETSOLVE_LINK_DTYPE = np.dtype([("g", np.float64), ("q", np.float64)])
NETSOLVE_INLET, NETSOLVE_OUTLET, NETSOLVE_SHORTED = 1, 2, 4
NETSOLVE_COUNTERS = ("regions", "links", "inlet_regions", "outlet_regions", "shorted_regions", "free_regions", "iterations", "status",
                     "flowing_links", "strongest_link")
NETSOLVE_SUMS = ("Q_in", "Q_out", "rz0", "rz")


def write_netsolve_files(directory, nFile, lx, ly, n, merge, level, frm, band, to, links, solved, region_body, regions, counts, sums, t,
                         precision="f64"):
    """netsolve_regions%.6i.dat, netsolve_links%.6i.dat and one appended line of netsolve.data (include/lbmdem_hip.h spells the
    three formats out) from the network's links of the level (NET_LINK_DTYPE) and their solution (NETSOLVE_LINK_DTYPE), per region
    its (root) body number and its record (NETSOLVE_REGION_DTYPE), the ten counts and the four sums (dicts of NETSOLVE_COUNTERS
    and NETSOLVE_SUMS, or sequences) and the time of the line; n: the grain count of the first lines. Host only."""
    li = np.ascontiguousarray(links, dtype=NET_LINK_DTYPE).reshape(-1)
    so = np.ascontiguousarray(solved, dtype=NETSOLVE_LINK_DTYPE).reshape(-1)
    rb = np.ascontiguousarray(region_body, dtype=np.int32).reshape(-1)
    rg = np.ascontiguousarray(regions, dtype=NETSOLVE_REGION_DTYPE).reshape(-1)
    if isinstance(counts, dict):
        counts = [counts[k] for k in NETSOLVE_COUNTERS]
    if isinstance(sums, dict):
        sums = [sums[k] for k in NETSOLVE_SUMS]
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    sm = np.ascontiguousarray(sums, dtype=np.float64).reshape(-1)
    if len(cnt) != len(NETSOLVE_COUNTERS) or len(sm) != len(NETSOLVE_SUMS):
        raise LbmDemError(-1, "write_netsolve_files: ten counts and four sums")
    _chk(load_library(precision).lbmdem_write_netsolve_files(
        os.fsencode(directory), int(nFile), int(lx), int(ly), int(n), int(merge), int(level), int(frm), int(band), int(to),
        _vp(li) if len(li) else None, len(li), _vp(so) if len(so) else None, len(so), _vp(rb) if len(rb) else None, len(rb),
        _vp(rg) if len(rg) else None, len(rg), _vp(cnt), _vp(sm), float(t)))


# struct lbmdem_coarse_cell: one cell of the coarse-grained fields (LbmDem.coarse_fields), 25 doubles
COARSE_FIELDS = ("nodes fluid_nodes grain_nodes wall_nodes sum_rho sum_jx sum_jy sum_P grains sum_m sum_mv1 sum_mv2 sum_Iw "
                 "ke_x ke_y ke_teta sum_fhf1 sum_fhf2 sum_fhf3 sum_z sum_p M11 M12 M21 M22").split()
COARSE_DTYPE = np.dtype([(name, np.float64) for name in COARSE_FIELDS])


def coarse_grid(lx, ly, cw, ch, precision="f64"):
    """(ncx, ncy) of cells of cw x ch nodes over an lx x ly lattice: (lx + cw - 1) // cw, (ly + ch - 1) // ch. Host only."""
    ncx, ncy = C.c_int(0), C.c_int(0)
    _chk(load_library(precision).lbmdem_coarse_grid(int(lx), int(ly), int(cw), int(ch), C.byref(ncx), C.byref(ncy)))
    return int(ncx.value), int(ncy.value)


def write_coarse_files(directory, nFile, lx, ly, cw, ch, cells, outside=0, contacts_valid=0, precision="f64"):
    """coarse%.6i.dat: "# cw %d ch %d ncx %d ncy %d outside %ld contacts %d", then one line per cell, cx outer and cy inner:
    "%d %d" and the 25 members of COARSE_DTYPE as " %le". `cells`: (ncx, ncy) of COARSE_DTYPE. Host only."""
    ncx, ncy = coarse_grid(lx, ly, cw, ch, precision)
    cells = np.ascontiguousarray(cells, dtype=COARSE_DTYPE)
    if cells.shape != (ncx, ncy):
        raise LbmDemError(-1, f"write_coarse_files: cells must have shape {(ncx, ncy)}, not {cells.shape}")
    _chk(load_library(precision).lbmdem_write_coarse_files(os.fsencode(directory), int(nFile), int(lx), int(ly), int(cw), int(ch),
                                                           _vp(cells), int(outside), int(contacts_valid)))


# the flow fields (LbmDem.flow_fields): the bits of the mask in plane order, LBMDEM_FLOW_*
FLOW_NAMES = ("ux", "uy", "vort", "div", "nxx", "nxy", "gdot", "diss")
FLOW_UX, FLOW_UY, FLOW_VORT, FLOW_DIV, FLOW_NXX, FLOW_NXY, FLOW_GDOT, FLOW_DISS = (1 << k for k in range(8))
FLOW_ALL = 255
FLOW_SUMS = ("n_fluid", "sum_rho", "sum_ke", "sum_diss", "sum_enstrophy", "max_u2", "max_gdot", "max_abs_div")


def flow_plane_names(mask):
    """the fields a mask selects, in plane order (ascending bit)"""
    mask = int(mask)
    if mask <= 0 or mask & ~FLOW_ALL:
        raise LbmDemError(-1, f"flow fields: bad mask {mask}")
    return [name for k, name in enumerate(FLOW_NAMES) if mask >> k & 1]


def write_flow_files(directory, nFile, ux, uy, vort, gdot, diss, precision="f64"):
    """flow%.6i.vtk from five planes (lx, ly) of doubles: the binary rectilinear-mesh format of write_vtk's files with the
    point data fluid_velocity_lb (ux, uy, 0), vorticity, shear_rate, dissipation, each value cast to float. Host only."""
    planes = [np.ascontiguousarray(p, dtype=np.float64) for p in (ux, uy, vort, gdot, diss)]
    if planes[0].ndim != 2 or any(p.shape != planes[0].shape for p in planes):
        raise LbmDemError(-1, "write_flow_files: five planes of one shape (lx, ly)")
    lx, ly = planes[0].shape
    _chk(load_library(precision).lbmdem_write_flow_files(os.fsencode(directory), int(nFile), lx, ly, *(_vp(p) for p in planes)))


TRACER_COUNTERS = ("tracers", "advances", "hook_advances")   # LbmDem.tracer_stats


def write_tracers_files(directory, nFile, lx, xy, uvo, precision="f64"):
    """tracers%.6i.vtk, legacy binary POLYDATA, from positions (n, 2) in node coordinates and their sample (n, 3) U, V, owner:
    one vertex per tracer at the coordinates of the frames' mesh ((float)px * (float)(1 / lx), ...), the point data
    tracer_velocity_lb and tracer_owner. n = 0 writes a valid empty file. Host only."""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    uvo = np.ascontiguousarray(uvo, dtype=np.float64).reshape(-1, 3)
    if len(xy) != len(uvo):
        raise LbmDemError(-1, "write_tracers_files: positions (n, 2) and their sample (n, 3)")
    n = len(xy)
    _chk(load_library(precision).lbmdem_write_tracers_files(os.fsencode(directory), int(nFile), int(lx), n,
                                                            _vp(xy) if n else None, _vp(uvo) if n else None))


SCALAR_SUMS = ("n_fluid", "sum_C", "sum_C2", "min_C", "max_C")   # LbmDem.scalar_sums
SCALAR_COUNTERS = ("present", "steps", "hook_steps")             # LbmDem.scalar_stats


def write_scalar_files(directory, nFile, C_plane, precision="f64"):
    """scalar%.6i.vtk, legacy binary STRUCTURED_POINTS on the nodes of the frames' mesh, from the concentration plane [lx][ly]:
    (float)C of every node, big-endian, x fastest (include/lbmdem_hip.h spells the layout out). Host only."""
    plane = np.ascontiguousarray(C_plane, dtype=np.float64)
    if plane.ndim != 2:
        raise LbmDemError(-1, "write_scalar_files: a plane of shape (lx, ly)")
    lx, ly = plane.shape
    _chk(load_library(precision).lbmdem_write_scalar_files(os.fsencode(directory), int(nFile), lx, ly, _vp(plane)))


# time-averaged flow statistics (LbmDem.begin_mean ...): the accumulators of a window, the derived fields, the profile's rows
MEAN_U, MEAN_UU, MEAN_RHO, MEAN_DISS, MEAN_GRAIN = (1 << k for k in range(5))
MEAN_ALL = 31
MEAN_PLANES = (("Sux", "Suy"), ("Sxx", "Sxy", "Syy"), ("Srho", "Srho2"), ("Sdiss", "Sgdot"), ("Sgux", "Sguy"))   # per bit
MEANF_NAMES = ("phi", "solid", "mux", "muy", "rxx", "rxy", "ryy", "mrho", "vrho", "mdiss", "mgdot", "gux", "guy")
(MEANF_PHI, MEANF_SOLID, MEANF_UX, MEANF_UY, MEANF_RXX, MEANF_RXY, MEANF_RYY, MEANF_RHO, MEANF_VRHO, MEANF_DISS, MEANF_GDOT,
 MEANF_GUX, MEANF_GUY) = (1 << k for k in range(13))
MEANF_ALL = 8191
MEAN_PROFILE_ROWS = MEANF_NAMES + ("nf",)
MEAN_COUNTERS = ("present", "mask", "samples", "hook_steps", "bytes")   # LbmDem.mean_stats
# LBMDEM_CKPT_*: the optional state a checkpoint carries (LbmDem.set_checkpoint_contents, LbmDem.checkpoint_contents)
CKPT_TRACERS, CKPT_SCALAR, CKPT_MEAN, CKPT_ALL = 1, 2, 4, 7
CKPT_CONTENTS = ("mask", "tracers", "scalar_steps", "mean_mask", "mean_samples")


def mean_plane_names(mask):
    """the accumulator planes a window's mask selects, in plane order"""
    mask = int(mask)
    if mask <= 0 or mask & ~MEAN_ALL:
        raise LbmDemError(-1, f"time-averaged statistics: bad mask {mask}")
    return [name for k, group in enumerate(MEAN_PLANES) if mask >> k & 1 for name in group]


def mean_field_names(fmask):
    """the derived fields a field mask selects, in plane order (ascending bit)"""
    fmask = int(fmask)
    if fmask <= 0 or fmask & ~MEANF_ALL:
        raise LbmDemError(-1, f"time-averaged statistics: bad field mask {fmask}")
    return [name for k, name in enumerate(MEANF_NAMES) if fmask >> k & 1]


def write_mean_files(directory, nFile, samples, phi, mux, muy, rxx, rxy, ryy, mrho, profile14, precision="f64"):
    """mean%.6i.vtk (the format of flow%.6i.vtk: mean_fluid_velocity_lb, fluid_fraction, fluctuation_energy = 0.5 * (rxx + ryy),
    reynolds_xy = rxy, mean_density) and mean_profile%.6i.dat (per y: y, samples, the thirteen profile rows over lx) from seven
    planes (lx, ly) and the profile (14, ly). Host only."""
    planes = [np.ascontiguousarray(p, dtype=np.float64) for p in (phi, mux, muy, rxx, rxy, ryy, mrho)]
    if planes[0].ndim != 2 or any(p.shape != planes[0].shape for p in planes):
        raise LbmDemError(-1, "write_mean_files: seven planes of one shape (lx, ly)")
    lx, ly = planes[0].shape
    prof = np.ascontiguousarray(profile14, dtype=np.float64)
    if prof.shape != (len(MEAN_PROFILE_ROWS), ly):
        raise LbmDemError(-1, f"write_mean_files: a profile of shape ({len(MEAN_PROFILE_ROWS)}, ly)")
    _chk(load_library(precision).lbmdem_write_mean_files(os.fsencode(directory), int(nFile), lx, ly, int(samples),
                                                         *(_vp(p) for p in planes), _vp(prof)))


class _DeviceBlock:
    """a block of device memory -- float64, or int32 with typestr "<i4" -- as torch.as_tensor reads it (the CUDA array interface):
    a view, nothing is copied"""

    def __init__(self, ptr, shape, typestr="<f8"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


def write_densities_host(directory, nFile, f, obst, t=0.0, rho_moy=1000.0):
    """write_densities (main.c:482-566) over host arrays f[lx][ly][9] and obst[lx][ly]: densities%.6i.vtk and
    pressure_base%.6i.dat, the reference's loops with one fprintf per value. Host only."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    obst = np.ascontiguousarray(obst, dtype=np.int32)
    if f.ndim != 3 or f.shape[2] != 9 or obst.shape != f.shape[:2]:
        raise LbmDemError(-1, "write_densities_host: f must be [lx][ly][9] and obst [lx][ly]")
    _chk(load_library().lbmdem_write_densities_host(os.fsencode(directory), int(nFile), f.shape[0], f.shape[1], float(t),
                                                    float(rho_moy), _vp(f), _vp(obst)))


def format_fixed4(values):
    """bytes: every value as printf's "%.4lf" followed by a newline, made by the formatter the device uses (finite values
    below 1e9 in magnitude). Host only."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    out = np.empty(17 * len(v) + 1, np.uint8)
    n = C.c_long(0)
    _chk(load_library().lbmdem_format_fixed4(_vp(v), len(v), _vp(out), len(out), C.byref(n)))
    return out[:n.value].tobytes()


DENSITIES_COUNTERS = ("pressure_bytes", "velocity_bytes", "bands", "refused_nodes")
DEM_ROW_DOUBLES = 28   # LBMDEM_DEM_ROW_DOUBLES


def write_dem_rows(directory, nFile, rows, stats22, forces=True, lx=0, ly=0):
    """DEM%06d.dat, one line appended to stats.data and (forces) DEM%06d.ps from a table's rows, (n, 28): r x1 x2 x3 v1 v2 v3
    a1 a2 a3 fhf1 fhf2 fhf3 p s ESE fr ifr ice slip rw fm M11 M12 M21 M22 z zz, and the 22 numbers of the stats line. Host only."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    st = np.ascontiguousarray(stats22, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != DEM_ROW_DOUBLES or st.shape != (22,):
        raise LbmDemError(-1, f"write_dem_rows: rows must be (n, {DEM_ROW_DOUBLES}) and stats22 (22,)")
    _chk(load_library().lbmdem_write_dem_rows(os.fsencode(directory), int(nFile), rows.shape[0], _vp(rows), _vp(st),
                                              int(bool(forces)), int(lx), int(ly)))


def exported_symbols():
    """Names the public header declares (used by the CPU test that checks the ABI surface)."""
    import re
    txt = open(HEADER_PATH).read()
    return sorted(set(re.findall(r"\b(lbmdem_[a-z_0-9]+)\s*\(", txt)))


def _chk(rc):
    if rc != 0:
        msg = load_library().lbmdem_last_error().decode(errors="replace")
        if _lib_sp is not None:      # the float build keeps its own error text
            sp = _lib_sp.lbmdem_last_error().decode(errors="replace")
            msg = sp if not msg else (msg if not sp else f"{msg} | f32 library: {sp}")
        raise LbmDemError(rc, msg)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def read_sample(path, precision="f64"):
    """read_sample (main.c:609-639) -> (r, x1, x2) in metres. precision "f32": parsed as the reference's
    -DSINGLE_PRECISION build parses it (text -> float, times the float 1e-3)."""
    L = load_library(precision)
    n = C.c_int(0)
    pr, p1, p2 = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
    _chk(L.lbmdem_read_sample(os.fsencode(path), C.byref(n), C.byref(pr), C.byref(p1), C.byref(p2)))
    out = tuple(np.ctypeslib.as_array(p, shape=(n.value,)).copy() for p in (pr, p1, p2))
    for p in (pr, p1, p2):
        L.lbmdem_free_host(C.cast(p, C.c_void_p))
    return out


def derive(lx, ly, r, scale=1.0, physics: Physics | None = None, precision="f64") -> Config:
    """Time-step derivation of main.c:1836-1860 (host arithmetic, bit-identical; "f32": in the float build's types)."""
    L = load_library(precision)
    cfg = Config()
    if physics is None:
        _chk(L.lbmdem_physics_defaults(C.byref(cfg.phys)))
    else:
        cfg.phys = physics
    r = np.ascontiguousarray(r, dtype=np.float64)
    _chk(L.lbmdem_derive(C.byref(cfg), int(lx), int(ly), float(scale), len(r), _vp(r)))
    cfg.x_begin, cfg.x_end, cfg.halo, cfg.device = 0, int(lx), 0, 0
    return cfg


COMM_ID_BYTES = 512


def vibration_schedule(cfg: Config, nbsteps0: int, n: int, precision="f64"):
    """The walls of a vibrating run (the reference's vib = 1, main.c:1700-1705) on sub-steps nbsteps0 .. nbsteps0 + n - 1,
    starting from cfg's clock and walls: [n][4] = t, Mgx, Mdx, the top wall's amp*freq*cos(freq*t). Host arithmetic only."""
    L = load_library(precision)
    out = np.zeros((max(int(n), 0), 4))
    _chk(L.lbmdem_vibration_schedule(C.byref(cfg), int(nbsteps0), int(n), _vp(out)))
    return out


def scene_schedule(cfg: Config, nbsteps0: int, n: int, duration: float = -1.0, fluid: bool = True, precision="f64"):
    """The events of n calls of renderScene() from step counter nbsteps0 in the reference's main loop (main.c:1697-1777,
    1880-1890), in order: [(kind, step, nfile)], kind one of SCENE_KINDS -- check_density's line, write_vtk, write_DEM +
    write_forces, the "steps" line, the stop (first step with step * dt > duration; duration < 0: none). Host arithmetic only."""
    L = load_library(precision)
    count = C.c_long(0)
    _chk(L.lbmdem_scene_schedule(C.byref(cfg), int(nbsteps0), int(n), float(duration), int(bool(fluid)), None, 0, C.byref(count)))
    ev = (SceneEvent * max(count.value, 1))()
    _chk(L.lbmdem_scene_schedule(C.byref(cfg), int(nbsteps0), int(n), float(duration), int(bool(fluid)), ev, count.value,
                                 C.byref(count)))
    return [(SCENE_KINDS[ev[k].kind], int(ev[k].step), int(ev[k].nfile)) for k in range(count.value)]


def comm_unique_id() -> bytes:
    """RCCL ids for one communicator group (rank 0 makes them, every rank gets the same bytes)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _chk(load_library().lbmdem_comm_unique_id(buf))
    return buf.raw


class Comm:
    """The library's own RCCL transport (lbmdem_comm_*): neighbour send/recv of the distributed-grain protocol, driven
    from C -- one call per renderScene batch, no Python on the step path."""

    def __init__(self, unique_id: bytes, rank: int, world: int, device: int):
        self._L = load_library()
        self._c = C.c_void_p()
        assert len(unique_id) == COMM_ID_BYTES
        _chk(self._L.lbmdem_comm_create(C.c_char_p(unique_id), int(rank), int(world), int(device), C.byref(self._c)))

    def close(self):
        if self._c:
            self._L.lbmdem_comm_destroy(self._c)
            self._c = C.c_void_p()

    def run(self, sim, n_dem_steps):
        _chk(self._L.lbmdem_comm_run(sim._h, self._c, int(n_dem_steps)))

    def allreduce_sum(self, values):
        a = np.ascontiguousarray(values, dtype=np.float64)
        _chk(self._L.lbmdem_comm_allreduce_sum(self._c, _vp(a), len(a)))
        return a

    def selftest(self, doubles=4096):
        _chk(self._L.lbmdem_comm_selftest(self._c, int(doubles)))


class LbmDem:
    """One simulation on one GPU (or one x-strip of it). Method names follow the reference.

    >>> sim = LbmDem.from_sample("a08d83.data", lx=600, ly=500)
    >>> for _ in range(240): sim.renderScene()
    >>> f = sim.f            # [lx][ly][9], the reference's host layout
    """

    def __init__(self, lx, ly, r, x1, x2, scale=1.0, device=0, strip=None, halo=0, physics=None, precision="f64",
                 origin=None):
        """precision "f32": the float build of the library (the reference's -DSINGLE_PRECISION mode, main.c:34-40): same
        methods, host arrays stay float64 (holding float values); step path and state transfers only.
        origin = (Mgx, Mby): the left and bottom walls of the config handed to lbmdem_create, where the reference's
        initialisation has 0, 0 (a restart of a shaken box finds its left wall off zero the same way)."""
        L = load_library(precision)
        self._L = L
        self.precision = precision
        self._h = C.c_void_p()
        r = np.ascontiguousarray(r, dtype=np.float64)
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        x2 = np.ascontiguousarray(x2, dtype=np.float64)
        if not (len(r) == len(x1) == len(x2)) or len(r) < 1:
            raise LbmDemError(-1, "r, x1, x2 must be equally long, at least one grain "
                                  "(the reference cannot run with 0 grains either: main.c:220)")
        cfg = derive(lx, ly, r, scale, physics, precision)
        cfg.device = int(device)
        if strip is not None:
            cfg.x_begin, cfg.x_end, cfg.halo = int(strip[0]), int(strip[1]), int(halo)
        if origin is not None:
            cfg.Mgx, cfg.Mby = float(origin[0]), float(origin[1])
        self.cfg = cfg
        self.lx, self.ly, self.n = int(lx), int(ly), len(r)
        _chk(L.lbmdem_create(C.byref(cfg), _vp(r), _vp(x1), _vp(x2), C.byref(self._h)))

    def checkpoint_save(self, path):
        _chk(self._L.lbmdem_checkpoint_save(self._h, os.fsencode(path)))

    @classmethod
    def checkpoint_load(cls, path, device=0):
        """Restart: a new simulation continuing bit-identically from a checkpoint."""
        L = load_library()
        self = cls.__new__(cls)
        self._L, self._h = L, C.c_void_p()
        _chk(L.lbmdem_checkpoint_load(os.fsencode(path), int(device), C.byref(self._h)))
        self.cfg = self.config()
        self.lx, self.ly, self.n = self.cfg.lx, self.cfg.ly, self.cfg.nbgrains
        return self

    def set_async_checkpoint(self, slots=1):
        """Checkpoints in the background: `slots` checkpoint slots (1..2) of device staging + pinned host memory of the file's
        size; the writer thread and copy stream are those of set_async_output. 0 switches it off again (writes what is queued
        first)."""
        _chk(self._L.lbmdem_set_async_checkpoint(self._h, int(slots)))

    def checkpoint_save_async(self, path):
        """checkpoint_save without the wait: one snapshot kernel on the step stream, then copy and file I/O behind the run's back.
        The file is checkpoint_save's followed by a digest trailer (checkpoint_verify); it replaces `path` atomically once
        complete (output_drain() returns when it has). Waits for a free slot when all are in flight."""
        _chk(self._L.lbmdem_checkpoint_save_async(self._h, os.fsencode(path)))

    def set_checkpoint_every(self, every_substeps, path=None):
        """run_scene saves a checkpoint to `path` whenever the step counter reaches a multiple of `every_substeps` -- in the
        background when set_async_checkpoint has made slots, else synchronously; always by way of path + ".tmp" and rename.
        0 switches it off."""
        _chk(self._L.lbmdem_set_checkpoint_every(self._h, int(every_substeps), os.fsencode(path) if path is not None else None))

    def output_stats_checkpoint(self):
        """dict: checkpoints queued / written / failed, calls that waited for a slot; ms the caller waited for a slot, the writer
        waited for copies, the writer spent in file I/O, callers were held in checkpoint_save_async behind their slot"""
        return self._output_stats(self._L.lbmdem_output_stats_checkpoint, "ms_hold")

    def _output_stats(self, fn, last_key):
        """the four counters and four times of one kind of background job; the last time means something else for each kind"""
        c = np.zeros(4, np.int64); m = np.zeros(4)
        _chk(fn(self._h, _vp(c), _vp(m)))
        return {"queued": int(c[0]), "written": int(c[1]), "failed": int(c[2]), "slot_waits": int(c[3]),
                "ms_slot_wait": float(m[0]), "ms_copy_wait": float(m[1]), "ms_io": float(m[2]), last_key: float(m[3])}

    @staticmethod
    def checkpoint_verify(path):
        """Recompute every section of a checkpoint file against its digest trailer (host only, no device). -> True when the file
        has a trailer and matches it, False for a file without one (checkpoint_save's); raises naming the first section that
        differs, or for a trailer that is cut short."""
        has = C.c_int(0)
        _chk(load_library().lbmdem_checkpoint_verify(os.fsencode(path), C.byref(has)))
        return bool(has.value)

    def set_checkpoint_contents(self, mask=CKPT_ALL):
        """Every save of this handle (checkpoint_save, checkpoint_save_async, run_scene's cadence) adds what of CKPT_TRACERS |
        CKPT_SCALAR | CKPT_MEAN it has at that moment; checkpoint_load restores whatever a file holds. 0: off (the default),
        and then, or with nothing selected present, the file is the plain file byte for byte."""
        _chk(self._L.lbmdem_set_checkpoint_contents(self._h, int(mask)))

    @staticmethod
    def checkpoint_contents(path):
        """dict: what a checkpoint file carries beyond the plain state -- mask (CKPT_*), tracers, scalar_steps, mean_mask,
        mean_samples; all 0 for a plain file. Host only, no device."""
        out = np.zeros(5, np.int64)
        _chk(load_library().lbmdem_checkpoint_contents(os.fsencode(path), _vp(out)))
        return dict(zip(CKPT_CONTENTS, (int(v) for v in out)))

    @staticmethod
    def checkpoint_digest(data):
        """(S1, S2) of a byte string as a checkpoint section: of its little-endian uint64 words w_i (the last zero-padded)
        S1 = sum w_i, S2 = sum (i + 1) w_i, both mod 2**64. Host only."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        out = np.zeros(2, np.uint64)
        _chk(load_library().lbmdem_checkpoint_digest(_vp(buf) if buf.size else None, int(buf.size), _vp(out)))
        return int(out[0]), int(out[1])

    @classmethod
    def from_sample(cls, path, lx, ly, **kw):
        r, x1, x2 = read_sample(path)
        return cls(lx, ly, r, x1, x2, **kw)

    def close(self):
        if getattr(self, "_h", None):
            self._L.lbmdem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- the reference's routines -------------------------------------------------------------
    def renderScene(self, n=1):
        """n x renderScene() (main.c:1697-1765)."""
        _chk(self._L.lbmdem_run(self._h, int(n)))

    def run_scene(self, n, outdir=None, fluid=True, duration=-1.0, comm=None):
        """The reference's main loop (main.c:1879-1890) for n x renderScene(), or fewer when step * dt > duration ends it
        (duration < 0: never): check_density's console lines, write_vtk / write_DEM / write_forces into `outdir` at the
        reference's cadences (None: no files), the "steps" lines; the sub-steps between two of those in one call of the run
        loop. fluid=False: the reference without `#define _FLUIDE_`. -> (console lines, dict(steps_done, nfile, stopped,
        energies8, last_density)). The header line of stats.data is the caller's."""
        lines = []
        say = _SAY(lambda user, line: lines.append(line.decode(errors="replace")))
        sc = Scene(os.fsencode(outdir) if outdir is not None else None, int(bool(fluid)), float(duration), say, None)
        res = SceneResult()
        _chk(self._L.lbmdem_run_scene(self._h, comm._c if comm is not None else None, int(n), C.byref(sc), C.byref(res)))
        return lines, dict(steps_done=int(res.steps_done), nfile=int(res.nfile), stopped=bool(res.stopped),
                           energies8=tuple(res.energies8), last_density=float(res.last_density))

    def run_dem(self, n=1):
        """n x (Verlet rebuild when due; DEM sub-step) -- renderScene without its fluid step."""
        _chk(self._L.lbmdem_run_dem(self._h, int(n)))

    def renderScene_dry(self, n=1):
        """n x renderScene() of the reference compiled without `#define _FLUIDE_` (main.c:16, 1709-1719): DEM only -- no
        fluid step, the hydrodynamic forces keep their values (0 from the start)."""
        self.run_dem(n)

    def lbm_step(self):
        """reinit_obst_density + obst_construction + collision_streaming + forces_fluid (main.c:1711-1717)."""
        _chk(self._L.lbmdem_lbm_step(self._h))

    def obst_construction(self):
        _chk(self._L.lbmdem_obst_construction(self._h))

    def collision_streaming(self):
        """reinit_obst_density (with the previous obstacle map) + collision_streaming."""
        _chk(self._L.lbmdem_collide_stream(self._h))

    def collision_streaming_edges(self):
        """First part of a split collision_streaming: the owned rows a neighbouring strip needs."""
        _chk(self._L.lbmdem_collide_stream_part(self._h, 1))

    def collision_streaming_interior(self):
        """Second part: all other owned rows (runs while the halo rows travel)."""
        _chk(self._L.lbmdem_collide_stream_part(self._h, 2))

    def forces_fluid(self):
        _chk(self._L.lbmdem_forces_fluid(self._h))

    def initVerlet(self):
        """initVerlet + VerletWall (main.c:1519-1594)."""
        _chk(self._L.lbmdem_verlet_rebuild(self._h))

    VerletWall = initVerlet

    def dem_substep(self):
        """the integrator + acceleration_grains block of renderScene (main.c:1733-1764)."""
        _chk(self._L.lbmdem_dem_substep(self._h))

    def final_density(self, sum_in=0.0):
        """check_density / final_density (main.c:1249-1273) with the reference's bits: the serial chain over f[x][y][q],
        continued from `sum_in` over the owned rows. `self.density_rows_replayed` = rows added element by element."""
        s, n = C.c_double(0), C.c_int(0)
        _chk(self._L.lbmdem_total_density_serial(self._h, C.c_double(sum_in), C.byref(s), C.byref(n)))
        self.density_rows_replayed = n.value
        return s.value

    check_density = final_density

    def total_density_tree(self):
        """the same sum in tree order (one pass, last bits differ from the reference's)"""
        s = C.c_double(0)
        _chk(self._L.lbmdem_total_density(self._h, C.byref(s)))
        return s.value

    # ---- state ----------------------------------------------------------------------------------
    @property
    def nbsteps(self):
        return int(self._L.lbmdem_nbsteps(self._h))

    @nbsteps.setter
    def nbsteps(self, v):
        _chk(self._L.lbmdem_set_nbsteps(self._h, int(v)))

    @property
    def f(self):
        out = np.zeros((self.lx, self.ly, 9))
        _chk(self._L.lbmdem_download_f(self._h, _vp(out)))
        return out

    @f.setter
    def f(self, value):
        a = np.ascontiguousarray(value, dtype=np.float64)
        if a.shape != (self.lx, self.ly, 9):
            raise LbmDemError(-1, f"f must have shape {(self.lx, self.ly, 9)}")
        _chk(self._L.lbmdem_upload_f(self._h, _vp(a)))

    def download_f_into(self, out):
        _chk(self._L.lbmdem_download_f(self._h, _vp(out)))

    @property
    def obst(self):
        out = np.zeros((self.lx, self.ly), dtype=np.int32)
        _chk(self._L.lbmdem_download_obst(self._h, _vp(out)))
        return out

    # the boundary-link export: act, delta and obst_writing's files of the most recent rasterisation (include/lbmdem_hip.h)
    def geometry_stats(self):
        """-> dict of GEOMETRY_COUNTERS: solid interior nodes, active solid nodes, effective links, links with 0 < delta < 1/2,
        links with delta >= 1/2, solid -> solid slots at active nodes"""
        c = np.zeros(6, np.int64)
        _chk(self._L.lbmdem_geometry_stats(self._h, _vp(c)))
        return dict(zip(GEOMETRY_COUNTERS, (int(v) for v in c)))

    def download_act(self):
        out = np.zeros((self.lx, self.ly), dtype=np.int32)
        _chk(self._L.lbmdem_download_act(self._h, _vp(out)))
        return out

    def download_links(self):
        """the effective links in the order of links.dat (y outer, x inner, q = 1..8): structured array of LINK_DTYPE"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_download_links(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=LINK_DTYPE)
        if n.value:
            _chk(self._L.lbmdem_download_links(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def download_geometry_obst(self):
        """the map the three calls above describe (after a run that has painted for the coming fluid step: that new map)"""
        out = np.zeros((self.lx, self.ly), dtype=np.int32)
        _chk(self._L.lbmdem_download_geometry_obst(self._h, _vp(out)))
        return out

    def write_obst(self, directory="."):
        _chk(self._L.lbmdem_write_obst(self._h, os.fsencode(directory)))

    # the contact network export: the contacts of the last sub-step, when it was a table sub-step (include/lbmdem_hip.h)
    def contact_stats(self):
        """-> dict of CONTACT_COUNTERS: list entries i < j, touching pairs, those that took the Coulomb clamp, those with fn == 0,
        wall contacts, grains with at least one record"""
        c = np.zeros(6, np.int64)
        _chk(self._L.lbmdem_contact_stats(self._h, _vp(c)))
        return dict(zip(CONTACT_COUNTERS, (int(v) for v in c)))

    def download_contacts(self):
        """structured array of CONTACT_DTYPE: the pair records (i < j, i ascending, j ascending), then the wall records (grain
        ascending, WALL_B, WALL_T, WALL_L, WALL_R within a grain)"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_download_contacts(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=CONTACT_DTYPE)
        if n.value:
            _chk(self._L.lbmdem_download_contacts(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def write_contacts(self, directory=".", nFile=0):
        """contacts%.6i.dat and DEM%.6i_chains.ps of the last table sub-step"""
        _chk(self._L.lbmdem_write_contacts(self._h, os.fsencode(directory), int(nFile)))

    def set_contacts_output(self, on=True):
        """run_scene writes the contact files at every DEM event, right behind write_DEM / write_forces"""
        _chk(self._L.lbmdem_set_contacts_output(self._h, 1 if on else 0))

    # force chains: clusters, coordination and rattlers of the contact net of the last table sub-step (include/lbmdem_hip.h)
    def clusters(self, fmin=1.0, relative=True, zmin=2):
        """the cluster analysis of the records at or above the threshold -- fmin, or fmin times the mean of the positive pair
        forces when relative -- with the core that is left when grains of fewer than zmin contacts are removed over and over
        -> (dict of CLUSTER_COUNTERS, the threshold)"""
        c = np.zeros(len(CLUSTER_COUNTERS), np.int64)
        thr = C.c_double(0.0)
        _chk(self._L.lbmdem_cluster_compute(self._h, float(fmin), int(bool(relative)), int(zmin), _vp(c), C.byref(thr)))
        return dict(zip(CLUSTER_COUNTERS, (int(v) for v in c))), float(thr.value)

    def cluster_grains(self):
        """-> dict of the per-grain results of the last clusters(): label (the smallest grain of the component), degree, core
        (1: not removed), walls (bit 0 .. 3: a selected contact with the bottom, top, left, right wall); int32 arrays [n]"""
        out = {k: np.zeros(self.n, np.int32) for k in ("label", "degree", "core", "walls")}
        _chk(self._L.lbmdem_download_cluster_grains(self._h, *(_vp(out[k]) for k in ("label", "degree", "core", "walls"))))
        return out

    def cluster_grains_tensors(self):
        """the same four as torch.int32 views of the handle's device memory, good until the next clusters()"""
        import torch
        p = [C.c_void_p() for _ in range(4)]
        _chk(self._L.lbmdem_cluster_grains_device(self._h, *(C.byref(q) for q in p)))
        dev = f"cuda:{self.cfg.device}"
        return {k: torch.as_tensor(_DeviceBlock(q.value, (self.n,), "<i4"), device=dev)
                for k, q in zip(("label", "degree", "core", "walls"), p)}

    def cluster_table(self):
        """structured array of CLUSTER_DTYPE: the components of two or more grains of the last clusters(), ascending label"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_download_clusters(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=CLUSTER_DTYPE)
        if n.value:
            _chk(self._L.lbmdem_download_clusters(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def cluster_rounds(self):
        """(rounds of the component loop, rounds of the core loop that removed a grain) of the last clusters()"""
        r = np.zeros(2, np.int32)
        _chk(self._L.lbmdem_cluster_rounds(self._h, _vp(r)))
        return int(r[0]), int(r[1])

    def write_clusters(self, directory=".", nFile=0, fmin=1.0, relative=True, zmin=2):
        """clusters%.6i.dat, cluster_table%.6i.dat, DEM%.6i_clusters.ps and a line of clusters.data of the last table sub-step"""
        _chk(self._L.lbmdem_write_clusters(self._h, os.fsencode(directory), int(nFile), float(fmin), int(bool(relative)), int(zmin)))

    def set_clusters_output(self, on=True, fmin=1.0, relative=True, zmin=2):
        """run_scene writes the cluster files at every DEM event, behind the contact files"""
        _chk(self._L.lbmdem_set_clusters_output(self._h, 1 if on else 0, float(fmin), int(bool(relative)), int(zmin)))

    # packing structure: neighbour shells, g(r) and bond order of the grains where they are now (include/lbmdem_hip.h)
    def structure(self, rcut, nbins=64, shell=1.2, max_entries=2 ** 31 - 1):
        """the fixed-radius neighbour list within rcut, the pair histogram of nbins bins, the bonds within shell times the sum of
        two radii and the bond-order and fabric sums; max_entries = 0: counts and histogram only -> dict of STRUCTURE_COUNTERS"""
        c = np.zeros(len(STRUCTURE_COUNTERS), np.int64)
        _chk(self._L.lbmdem_structure_compute(self._h, float(rcut), int(nbins), float(shell), int(max_entries), _vp(c)))
        return dict(zip(STRUCTURE_COUNTERS, (int(v) for v in c)))

    def structure_grains(self):
        """structured array [n] of STRUCTURE_DTYPE of the last structure(): neighbours, bonds and the unnormalised sums c6, s6
        (psi6) and c2, s2 (fabric) over the bonded neighbours"""
        cols = {k: np.zeros(self.n, STRUCTURE_DTYPE[k]) for k in STRUCTURE_DTYPE.names}
        _chk(self._L.lbmdem_download_structure_grains(self._h, *(_vp(cols[k]) for k in STRUCTURE_DTYPE.names)))
        out = np.zeros(self.n, STRUCTURE_DTYPE)
        for k in STRUCTURE_DTYPE.names:
            out[k] = cols[k]
        return out

    def structure_tensors(self):
        """the same six as torch views (int32, float64) of the handle's device memory, good until the next structure()"""
        import torch
        p = [C.c_void_p() for _ in range(6)]
        _chk(self._L.lbmdem_structure_grains_device(self._h, *(C.byref(q) for q in p)))
        dev = f"cuda:{self.cfg.device}"
        return {k: torch.as_tensor(_DeviceBlock(q.value, (self.n,), "<i4" if STRUCTURE_DTYPE[k] == np.int32 else "<f8"), device=dev)
                for k, q in zip(STRUCTURE_DTYPE.names, p)}

    def structure_hist(self):
        """int64 [nbins]: the unordered neighbour pairs per bin of the last structure()"""
        nb = C.c_int(0)
        _chk(self._L.lbmdem_download_structure_hist(self._h, None, 0, C.byref(nb)))
        out = np.zeros(nb.value, np.int64)
        _chk(self._L.lbmdem_download_structure_hist(self._h, _vp(out), nb.value, C.byref(nb)))
        return out

    def structure_neighbours(self):
        """-> (offsets int32 [n + 1], nbr int32 [entries]): the symmetric list of the last structure(), every grain's neighbours
        ascending by index"""
        cnt = C.c_long(0)
        _chk(self._L.lbmdem_download_structure_neighbours(self._h, None, None, 0, C.byref(cnt)))
        off, nbr = np.zeros(self.n + 1, np.int32), np.zeros(cnt.value, np.int32)
        _chk(self._L.lbmdem_download_structure_neighbours(self._h, _vp(off), _vp(nbr) if cnt.value else None, cnt.value, C.byref(cnt)))
        return off, nbr

    def write_structure(self, directory=".", nFile=0, rcut=0.0, nbins=64, shell=1.2):
        """structure%.6i.dat, gr%.6i.dat and a line of structure.data of the grains where they are now"""
        _chk(self._L.lbmdem_write_structure(self._h, os.fsencode(directory), int(nFile), float(rcut), int(nbins), float(shell)))

    def set_structure_output(self, on=True, rcut=0.0, nbins=64, shell=1.2):
        """run_scene writes the structure files at every DEM event, behind the cluster files"""
        _chk(self._L.lbmdem_set_structure_output(self._h, 1 if on else 0, float(rcut), int(nbins), float(shell)))

    # Voronoi cells: the radical tessellation on top of the last structure()'s neighbour list (include/lbmdem_hip.h)
    def voronoi(self, rcut=None):
        """the cells of the grains where they are now, from the neighbour list of the last structure(); with rcut that compute is
        made first, structure(rcut, 1, 1.0) -> dict of VORONOI_COUNTERS"""
        if rcut is not None:
            self.structure(rcut, 1, 1.0)
        c = np.zeros(len(VORONOI_COUNTERS), np.int64)
        _chk(self._L.lbmdem_voronoi_compute(self._h, _vp(c)))
        return dict(zip(VORONOI_COUNTERS, (int(v) for v in c)))

    def voronoi_grains(self):
        """structured array [n] of VORONOI_DTYPE of the last voronoi(): a cell's area, perimeter, local solid fraction and largest
        squared vertex distance, its grain faces, wall bits, vertices and flags (VOR_COMPLETE, ...)"""
        cols = {k: np.zeros(self.n, VORONOI_DTYPE[k]) for k in VORONOI_DTYPE.names}
        _chk(self._L.lbmdem_download_voronoi_grains(self._h, *(_vp(cols[k]) for k in VORONOI_DTYPE.names)))
        out = np.zeros(self.n, VORONOI_DTYPE)
        for k in VORONOI_DTYPE.names:
            out[k] = cols[k]
        return out

    def voronoi_tensors(self):
        """the same eight as torch views (float64, int32) of the handle's device memory, good until the next voronoi()"""
        import torch
        p = [C.c_void_p() for _ in range(8)]
        _chk(self._L.lbmdem_voronoi_grains_device(self._h, *(C.byref(q) for q in p)))
        dev = f"cuda:{self.cfg.device}"
        return {k: torch.as_tensor(_DeviceBlock(q.value, (self.n,), "<i4" if VORONOI_DTYPE[k] == np.int32 else "<f8"), device=dev)
                for k, q in zip(VORONOI_DTYPE.names, p)}

    def voronoi_faces(self):
        """-> (foff int32 [n + 1], fsrc int32 [faces], flen float64 [faces]): every cell's faces in polygon order, the neighbour
        behind each (or -1 .. -4: the bottom, right, top and left wall) and its length"""
        cnt = C.c_long(0)
        _chk(self._L.lbmdem_download_voronoi_faces(self._h, None, None, None, 0, C.byref(cnt)))
        off, src, length = np.zeros(self.n + 1, np.int32), np.zeros(cnt.value, np.int32), np.zeros(cnt.value, np.float64)
        _chk(self._L.lbmdem_download_voronoi_faces(self._h, _vp(off), _vp(src) if cnt.value else None,
                                                   _vp(length) if cnt.value else None, cnt.value, C.byref(cnt)))
        return off, src, length

    def write_voronoi(self, directory=".", nFile=0, rcut=0.0):
        """voronoi%.6i.dat and a line of voronoi.data of the grains where they are now"""
        _chk(self._L.lbmdem_write_voronoi(self._h, os.fsencode(directory), int(nFile), float(rcut)))

    def set_voronoi_output(self, on=True, rcut=0.0):
        """run_scene writes the Voronoi files at every DEM event, behind the structure files"""
        _chk(self._L.lbmdem_set_voronoi_output(self._h, 1 if on else 0, float(rcut)))

    # strain fields: the grains where they are now against a marked reference state (include/lbmdem_hip.h)
    def strain_mark(self):
        """marks the grains where they are now, with the neighbour list of the last structure(), as the reference state ->
        the list entries copied"""
        cnt = C.c_long(0)
        _chk(self._L.lbmdem_strain_mark(self._h, C.byref(cnt)))
        return cnt.value

    def strain_clear(self):
        """no mark and no result any more"""
        _chk(self._L.lbmdem_strain_clear(self._h))

    def strain(self):
        """displacement, the fitted deformation gradient, D2min and the lost neighbours of every grain since the mark -> dict of
        STRAIN_COUNTERS"""
        c = np.zeros(len(STRAIN_COUNTERS), np.int64)
        _chk(self._L.lbmdem_strain_compute(self._h, _vp(c)))
        return dict(zip(STRAIN_COUNTERS, (int(v) for v in c)))

    def strain_grains(self):
        """structured array [n] of STRAIN_DTYPE of the last strain(): ux, uy, drot, the four entries of F, the unnormalised D2min,
        the marked neighbours used and lost, and flags (STRAIN_NONFINITE, STRAIN_FEW, STRAIN_DEGENERATE)"""
        cols = {k: np.zeros(self.n, STRAIN_DTYPE[k]) for k in STRAIN_DTYPE.names}
        _chk(self._L.lbmdem_download_strain_grains(self._h, *(_vp(cols[k]) for k in STRAIN_DTYPE.names)))
        out = np.zeros(self.n, STRAIN_DTYPE)
        for k in STRAIN_DTYPE.names:
            out[k] = cols[k]
        return out

    def strain_tensors(self):
        """the same eleven as torch views (float64, int32) of the handle's device memory, good until the next strain()"""
        import torch
        p = [C.c_void_p() for _ in range(11)]
        _chk(self._L.lbmdem_strain_grains_device(self._h, *(C.byref(q) for q in p)))
        dev = f"cuda:{self.cfg.device}"
        return {k: torch.as_tensor(_DeviceBlock(q.value, (self.n,), "<i4" if STRAIN_DTYPE[k] == np.int32 else "<f8"), device=dev)
                for k, q in zip(STRAIN_DTYPE.names, p)}

    def strain_reference(self):
        """the mark -> dict: x0, y0, th0 float64 [n], offsets int32 [n + 1], nbr int32 [entries], rc2, nbsteps"""
        cnt, rc2, nbs = C.c_long(0), C.c_double(0.), C.c_long(0)
        _chk(self._L.lbmdem_download_strain_reference(self._h, None, None, None, None, None, 0, C.byref(cnt), C.byref(rc2),
                                                      C.byref(nbs)))
        x0, y0, th0 = (np.zeros(self.n, np.float64) for _ in range(3))
        off, nbr = np.zeros(self.n + 1, np.int32), np.zeros(cnt.value, np.int32)
        _chk(self._L.lbmdem_download_strain_reference(self._h, _vp(x0), _vp(y0), _vp(th0), _vp(off), _vp(nbr) if cnt.value else None,
                                                      cnt.value, C.byref(cnt), C.byref(rc2), C.byref(nbs)))
        return {"x0": x0, "y0": y0, "th0": th0, "offsets": off, "nbr": nbr, "rc2": rc2.value, "nbsteps": nbs.value}

    def write_strain(self, directory=".", nFile=0, rcut=0.0, incremental=False):
        """strain%.6i.dat and a line of strain.data of the grains where they are now against the mark (made first, where there is
        none); incremental: a new mark afterwards"""
        _chk(self._L.lbmdem_write_strain(self._h, os.fsencode(directory), int(nFile), float(rcut), 1 if incremental else 0))

    def set_strain_output(self, on=True, rcut=0.0, incremental=False):
        """run_scene writes the strain files at every DEM event, behind the Voronoi files"""
        _chk(self._L.lbmdem_set_strain_output(self._h, 1 if on else 0, float(rcut), 1 if incremental else 0))

    # pore space: the connected components of the fluid phase of the map as it is now (include/lbmdem_hip.h)
    def pores(self, conn=8, map=None):
        """labels the fluid nodes of the handle's map -- or of `map`, (lx, ly) ints: -1 fluid, a grain's index, n the wall -- into
        components joined along 4 or 8 directions -> dict of PORE_COUNTERS"""
        c = np.zeros(len(PORE_COUNTERS), np.int64)
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, dtype=np.int32)
            if m.shape != (self.lx, self.ly):
                raise LbmDemError(-1, "pores: a map of shape (lx, ly)")
        _chk(self._L.lbmdem_pore_compute(self._h, int(conn), None if m is None else _vp(m), _vp(c)))
        return dict(zip(PORE_COUNTERS, (int(v) for v in c)))

    def pore_labels(self):
        """int32 (lx, ly) of the last pores(): the smallest index x * ly + y of a fluid node's component, -1 off the fluid"""
        out = np.empty((self.lx, self.ly), np.int32)
        _chk(self._L.lbmdem_download_pore_labels(self._h, _vp(out)))
        return out

    def pore_labels_tensor(self):
        """the same plane as a torch.int32 view (lx, sy) of the handle's device memory, sy the device's row pitch: node (x, y) at
        [x, y], the columns from ly on hold -1. Good until the next pores()."""
        import torch
        p, sy = C.c_void_p(), C.c_int(0)
        _chk(self._L.lbmdem_pore_labels_device(self._h, C.byref(p), C.byref(sy)))
        return torch.as_tensor(_DeviceBlock(p.value, (self.lx, sy.value), "<i4"), device=f"cuda:{self.cfg.device}")

    def pore_table(self):
        """structured array of PORE_DTYPE: the components of the last pores(), ascending label"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_download_pores(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=PORE_DTYPE)
        if n.value:
            _chk(self._L.lbmdem_download_pores(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def pore_grains(self):
        """-> dict of the per-grain results of the last pores(): wet (links into fluid), pore_min and pore_max (the smallest and
        largest label a grain borders, -1 without one); int32 arrays [n]"""
        out = {k: np.zeros(self.n, np.int32) for k in ("wet", "pore_min", "pore_max")}
        _chk(self._L.lbmdem_download_pore_grains(self._h, *(_vp(out[k]) for k in ("wet", "pore_min", "pore_max"))))
        return out

    def pore_grains_tensors(self):
        """the same three as torch.int32 views of the handle's device memory, good until the next pores()"""
        import torch
        p = [C.c_void_p() for _ in range(3)]
        _chk(self._L.lbmdem_pore_grains_device(self._h, *(C.byref(q) for q in p)))
        dev = f"cuda:{self.cfg.device}"
        return {k: torch.as_tensor(_DeviceBlock(q.value, (self.n,), "<i4"), device=dev)
                for k, q in zip(("wet", "pore_min", "pore_max"), p)}

    def write_pores(self, directory=".", nFile=0, conn=8, plane=False):
        """pore_table%.6i.dat, pore_grains%.6i.dat, a line of pores.data and (plane) pores%.6i.vtk of the map as it is now"""
        _chk(self._L.lbmdem_write_pores(self._h, os.fsencode(directory), int(nFile), int(conn), 1 if plane else 0))

    def set_pores_output(self, on=True, conn=8, plane=False):
        """run_scene writes the pore files at every DEM event, behind the Voronoi files"""
        _chk(self._L.lbmdem_set_pores_output(self._h, 1 if on else 0, int(conn), 1 if plane else 0))

    # pore clearance: the exact distance map of the map as it is now, its owners, the pore sizes and the throats (include/lbmdem_hip.h)
    def clearance(self, map=None, max_edges=0):
        """the squared distance from every fluid node of the handle's map -- or of `map`, (lx, ly) ints: -1 fluid, a grain's index,
        n the wall -- to the nearest position that is not fluid, with its owner, the histogram, the owners' table and the throats.
        max_edges: the most ridge edges to hold records for, 0: no limit -> dict of CLEARANCE_COUNTERS"""
        c = np.zeros(len(CLEARANCE_COUNTERS), np.int64)
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, dtype=np.int32)
            if m.shape != (self.lx, self.ly):
                raise LbmDemError(-1, "clearance: a map of shape (lx, ly)")
        _chk(self._L.lbmdem_clearance_compute(self._h, None if m is None else _vp(m), int(max_edges), _vp(c)))
        return dict(zip(CLEARANCE_COUNTERS, (int(v) for v in c)))

    def clearance_planes(self):
        """(d2, owner), int32 (lx, ly) each, of the last clearance(): the squared distance (0 off the fluid) and the nearest
        position's owner (the map itself off the fluid)"""
        d2, owner = np.empty((self.lx, self.ly), np.int32), np.empty((self.lx, self.ly), np.int32)
        _chk(self._L.lbmdem_download_clearance(self._h, _vp(d2), _vp(owner)))
        return d2, owner

    def clearance_tensors(self):
        """the same two planes as torch.int32 views (lx, sy) of the handle's device memory, sy the device's row pitch: node (x, y)
        at [x, y], the columns from ly on hold 0 (d2) and -1 (owner). Good until the next clearance()."""
        import torch
        p, q, sy = C.c_void_p(), C.c_void_p(), C.c_int(0)
        _chk(self._L.lbmdem_clearance_device(self._h, C.byref(p), C.byref(q), C.byref(sy)))
        dev = f"cuda:{self.cfg.device}"
        return {k: torch.as_tensor(_DeviceBlock(a.value, (self.lx, sy.value), "<i4"), device=dev) for k, a in (("d2", p), ("owner", q))}

    def clearance_hist(self):
        """int64 [kmax + 1] of the last clearance(): the fluid nodes per isqrt(d2), the pore-size distribution"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_download_clearance_hist(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int64)
        _chk(self._L.lbmdem_download_clearance_hist(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def clearance_owners(self):
        """-> dict of the per-owner results of the last clearance(), [n + 1] each, entry n the wall: owned (int64, the fluid nodes
        the owner has) and d2max (int32, the largest d2 among them, -1 without one)"""
        out = {"owned": np.zeros(self.n + 1, np.int64), "d2max": np.zeros(self.n + 1, np.int32)}
        _chk(self._L.lbmdem_download_clearance_owners(self._h, _vp(out["owned"]), _vp(out["d2max"])))
        return out

    def clearance_owner_tensors(self):
        """the same two as torch views (int64, int32) of the handle's device memory, good until the next clearance()"""
        import torch
        p, q = C.c_void_p(), C.c_void_p()
        _chk(self._L.lbmdem_clearance_owners_device(self._h, C.byref(p), C.byref(q)))
        dev = f"cuda:{self.cfg.device}"
        return {"owned": torch.as_tensor(_DeviceBlock(p.value, (self.n + 1,), "<i8"), device=dev),
                "d2max": torch.as_tensor(_DeviceBlock(q.value, (self.n + 1,), "<i4"), device=dev)}

    def throat_table(self):
        """structured array of THROAT_DTYPE: the throats of the last clearance(), ascending (lo, hi)"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_download_throats(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=THROAT_DTYPE)
        if n.value:
            _chk(self._L.lbmdem_download_throats(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def write_clearance(self, directory=".", nFile=0, plane=False):
        """throats%.6i.dat, clearance_hist%.6i.dat, clearance_owners%.6i.dat, a line of clearance.data and (plane)
        clearance%.6i.vtk of the map as it is now"""
        _chk(self._L.lbmdem_write_clearance(self._h, os.fsencode(directory), int(nFile), 1 if plane else 0))

    def set_clearance_output(self, on=True, plane=False):
        """run_scene writes the clearance files at every DEM event, behind the pore files"""
        _chk(self._L.lbmdem_set_clearance_output(self._h, 1 if on else 0, 1 if plane else 0))

    # pore network: the watershed of the clearance map -- bodies, links with their saddles, merged groups (include/lbmdem_hip.h)
    def network(self, map=None, merge=-1, max_edges=0):
        """the pore bodies of the handle's map -- or of `map`, (lx, ly) ints as clearance() takes them --, the links between them,
        the groups that bodies whose pass lies within `merge` of the lower summit's radius form (-1: no merging) and the links
        between those. Runs clearance() first where its result is not there. max_edges: the most edges between bodies to hold
        records for, 0: no limit -> dict of NETWORK_COUNTERS"""
        c = np.zeros(len(NETWORK_COUNTERS), np.int64)
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, dtype=np.int32)
            if m.shape != (self.lx, self.ly):
                raise LbmDemError(-1, "network: a map of shape (lx, ly)")
        _chk(self._L.lbmdem_network_compute(self._h, None if m is None else _vp(m), int(merge), int(max_edges), _vp(c)))
        return dict(zip(NETWORK_COUNTERS, (int(v) for v in c)))

    def network_planes(self):
        """(body, group), int32 (lx, ly) each, of the last network(): the body's number and the group's root body, -1 off the fluid"""
        body, group = np.empty((self.lx, self.ly), np.int32), np.empty((self.lx, self.ly), np.int32)
        _chk(self._L.lbmdem_download_network(self._h, _vp(body), _vp(group)))
        return body, group

    def network_tensors(self):
        """the same two planes as torch.int32 views (lx, sy) of the handle's device memory, sy the device's row pitch: node (x, y)
        at [x, y], the columns from ly on hold -1. Good until the next network()."""
        import torch
        p, q, sy = C.c_void_p(), C.c_void_p(), C.c_int(0)
        _chk(self._L.lbmdem_network_device(self._h, C.byref(p), C.byref(q), C.byref(sy)))
        dev = f"cuda:{self.cfg.device}"
        return {k: torch.as_tensor(_DeviceBlock(a.value, (self.lx, sy.value), "<i4"), device=dev) for k, a in (("body", p), ("group", q))}

    def _network_table(self, call, dtype, *lead):
        n = C.c_long(0)
        _chk(call(self._h, *lead, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=dtype)
        if n.value:
            _chk(call(self._h, *lead, _vp(out), n.value, C.byref(n)))
        return out

    def network_bodies(self):
        """structured array of NET_BODY_DTYPE: the bodies of the last network(), ascending by peak node"""
        return self._network_table(self._L.lbmdem_download_network_bodies, NET_BODY_DTYPE)

    def network_groups(self):
        """structured array of NET_GROUP_DTYPE: the groups of the last network(), ascending by root body"""
        return self._network_table(self._L.lbmdem_download_network_groups, NET_GROUP_DTYPE)

    def network_links(self, level=1):
        """structured array of NET_LINK_DTYPE: the links between bodies (level 0) or groups (1), ascending (lo, hi)"""
        return self._network_table(self._L.lbmdem_download_network_links, NET_LINK_DTYPE, int(level))

    def write_network(self, directory=".", nFile=0, merge=-1, plane=False):
        """network_bodies%.6i.dat, network_links%.6i.dat, network_groups%.6i.dat, a line of network.data and (plane)
        network%.6i.vtk of the map as it is now"""
        _chk(self._L.lbmdem_write_network(self._h, os.fsencode(directory), int(nFile), int(merge), 1 if plane else 0))

    def set_network_output(self, on=True, merge=-1, plane=False):
        """run_scene writes the network files at every DEM event, behind the clearance files"""
        _chk(self._L.lbmdem_set_network_output(self._h, 1 if on else 0, int(merge), 1 if plane else 0))

    # drainage: the largest disc that reaches each pore from a chosen side, over the pore network (include/lbmdem_hip.h)
    def drainage(self, frm, band=1, to=0, map=None, max_edges=0):
        """the widest path over the clearance map from the fluid nodes within `band` nodes of the sides `frm` (SIDE_B | SIDE_T |
        SIDE_L | SIDE_R) to every fluid node of the handle's map -- or of `map`, (lx, ly) ints as clearance() takes them --; `to`:
        the outlet sides the breakthrough size `critical` is taken over, 0: none. Runs network() first where its result is not
        there (max_edges: its budget) -> dict of DRAINAGE_COUNTERS"""
        c = np.zeros(len(DRAINAGE_COUNTERS), np.int64)
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, dtype=np.int32)
            if m.shape != (self.lx, self.ly):
                raise LbmDemError(-1, "drainage: a map of shape (lx, ly)")
        _chk(self._L.lbmdem_drainage_compute(self._h, None if m is None else _vp(m), int(frm), int(band), int(to), int(max_edges), _vp(c)))
        return dict(zip(DRAINAGE_COUNTERS, (int(v) for v in c)))

    def drainage_plane(self):
        """access, int32 (lx, ly), of the last drainage(): the squared size of the largest disc that reaches the node from the inlet,
        0 where none does and off the fluid"""
        access = np.empty((self.lx, self.ly), np.int32)
        _chk(self._L.lbmdem_download_drainage(self._h, _vp(access)))
        return access

    def drainage_tensor(self):
        """the same plane as a torch.int32 view (lx, sy) of the handle's device memory, sy the device's row pitch: node (x, y) at
        [x, y], the columns from ly on hold 0. Good until the next drainage()."""
        import torch
        p, sy = C.c_void_p(), C.c_int(0)
        _chk(self._L.lbmdem_drainage_device(self._h, C.byref(p), C.byref(sy)))
        return torch.as_tensor(_DeviceBlock(p.value, (self.lx, sy.value), "<i4"), device=f"cuda:{self.cfg.device}")

    def _drainage_table(self, call, dtype):
        n = C.c_long(0)
        _chk(call(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=dtype)
        if n.value:
            _chk(call(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def drainage_bodies(self):
        """int32 [bodies]: A, the largest access in each body of network_bodies(), 0 where the inlet does not reach"""
        return self._drainage_table(self._L.lbmdem_download_drainage_bodies, np.int32)

    def drainage_links(self):
        """int32 [links]: pass, the largest size that crosses each link of network_links(0) coming from the inlet"""
        return self._drainage_table(self._L.lbmdem_download_drainage_links, np.int32)

    def drainage_hist(self):
        """int64 [kmax + 1]: the fluid nodes per isqrt(access), entry for entry next to clearance_hist(); [0]: the unreached"""
        return self._drainage_table(self._L.lbmdem_download_drainage_hist, np.int64)

    def drainage_rounds(self):
        """the launches the relaxation of the last drainage() took, the quiet last one included"""
        r = C.c_int(0)
        _chk(self._L.lbmdem_drainage_rounds(self._h, C.byref(r)))
        return r.value

    def write_drainage(self, directory=".", nFile=0, frm=SIDE_T, band=1, to=0, plane=False):
        """drainage_curve%.6i.dat, drainage_bodies%.6i.dat, a line of drainage.data and (plane) drainage%.6i.vtk of the map as it
        is now"""
        _chk(self._L.lbmdem_write_drainage(self._h, os.fsencode(directory), int(nFile), int(frm), int(band), int(to), 1 if plane else 0))

    def set_drainage_output(self, on=True, frm=SIDE_T, band=1, to=0, plane=False):
        """run_scene writes the drainage files at every DEM event, behind the network files"""
        _chk(self._L.lbmdem_set_drainage_output(self._h, 1 if on else 0, int(frm), int(band), int(to), 1 if plane else 0))

    # geodesic: the length of the shortest path through the pore space from a chosen side (include/lbmdem_hip.h)
    def geodesic(self, frm, band=1, to=0, conn=8, min_d2=0, map=None, max_edges=0):
        """the shortest path of adjacent passable nodes -- fluid nodes with clearance d2 >= min_d2 -- from those within `band` nodes
        of the sides `frm` (SIDE_B | SIDE_T | SIDE_L | SIDE_R) to every passable node of the handle's map, or of `map`, (lx, ly)
        ints as clearance() takes them; an axis step costs GEO_UNIT = 5, a diagonal one (conn 8) 7. `to`: the outlet sides the
        backward distances, `shortest` and the corridor detour == 0 are taken over, 0: none. With min_d2 > 1 runs clearance()
        first where its result is not there (max_edges: its budget) -> dict of GEODESIC_COUNTERS"""
        c = np.zeros(len(GEODESIC_COUNTERS), np.int64)
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, dtype=np.int32)
            if m.shape != (self.lx, self.ly):
                raise LbmDemError(-1, "geodesic: a map of shape (lx, ly)")
        _chk(self._L.lbmdem_geodesic_compute(self._h, None if m is None else _vp(m), int(frm), int(band), int(to), int(conn), int(min_d2),
                                             int(max_edges), _vp(c)))
        return dict(zip(GEODESIC_COUNTERS, (int(v) for v in c)))

    def geodesic_planes(self):
        """-> dict(dist, back, detour), int32 (lx, ly) each, of the last geodesic(): the distance from the inlet, from the outlet,
        and dist + back - shortest; -1 where there is none"""
        out = {k: np.empty((self.lx, self.ly), np.int32) for k in ("dist", "back", "detour")}
        _chk(self._L.lbmdem_download_geodesic(self._h, _vp(out["dist"]), _vp(out["back"]), _vp(out["detour"])))
        return out

    def geodesic_tensors(self):
        """the same planes as torch.int32 views (lx, sy) of the handle's device memory, sy the device's row pitch: node (x, y) at
        [x, y], the columns from ly on hold -1. Good until the next geodesic()."""
        import torch
        p, sy = [C.c_void_p() for _ in range(3)], C.c_int(0)
        _chk(self._L.lbmdem_geodesic_device(self._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(sy)))
        return {k: torch.as_tensor(_DeviceBlock(q.value, (self.lx, sy.value), "<i4"), device=f"cuda:{self.cfg.device}")
                for k, q in zip(("dist", "back", "detour"), p)}

    def geodesic_profile(self):
        """structured array of GEO_LEVEL_DTYPE, one record per depth behind the inlet sides: the passable nodes, the reached ones,
        the sum of their dist, the least and the largest"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_download_geodesic_profile(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=GEO_LEVEL_DTYPE)
        if n.value:
            _chk(self._L.lbmdem_download_geodesic_profile(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def geodesic_rounds(self):
        """(forward, backward): the launches the two relaxations of the last geodesic() took, the quiet last ones included"""
        f, b = C.c_int(0), C.c_int(0)
        _chk(self._L.lbmdem_geodesic_rounds(self._h, C.byref(f), C.byref(b)))
        return f.value, b.value

    def write_geodesic(self, directory=".", nFile=0, frm=SIDE_T, band=1, to=0, conn=8, min_d2=0, plane=False):
        """geodesic_profile%.6i.dat, a line of geodesic.data and (plane) geodesic%.6i.vtk of the map as it is now"""
        _chk(self._L.lbmdem_write_geodesic(self._h, os.fsencode(directory), int(nFile), int(frm), int(band), int(to), int(conn),
                                           int(min_d2), 1 if plane else 0))

    def set_geodesic_output(self, on=True, frm=SIDE_T, band=1, to=0, conn=8, min_d2=0, plane=False):
        """run_scene writes the geodesic files at every DEM event, behind the drainage files"""
        _chk(self._L.lbmdem_set_geodesic_output(self._h, 1 if on else 0, int(frm), int(band), int(to), int(conn), int(min_d2),
                                                1 if plane else 0))

    # pore fluxes: the mass through every throat of the pore network in the last streaming step (include/lbmdem_hip.h)
    def netflux(self, merge=-1, level=0, map=None):
        """the mass that crossed every edge of adjacent fluid nodes of the handle's map -- or of `map`, (lx, ly) ints as
        clearance() takes them -- in the last streaming step, in units of 2^-32, summed per link and per region of the pore
        network at `merge` (level 0: the bodies, 1: the groups) and per section of the lattice. Runs network() first where its
        result at this merge is not there -> dict of NETFLUX_COUNTERS"""
        c = np.zeros(len(NETFLUX_COUNTERS), np.int64)
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, dtype=np.int32)
            if m.shape != (self.lx, self.ly):
                raise LbmDemError(-1, "netflux: a map of shape (lx, ly)")
        _chk(self._L.lbmdem_netflux_compute(self._h, None if m is None else _vp(m), int(merge), int(level), _vp(c)))
        return dict(zip(NETFLUX_COUNTERS, (int(v) for v in c)))

    def netflux_links(self):
        """structured array of NETFLUX_LINK_DTYPE, entry for entry next to network_links(level) of the last netflux()"""
        return self._drainage_table(self._L.lbmdem_download_netflux_links, NETFLUX_LINK_DTYPE)

    def netflux_regions(self):
        """structured array of NETFLUX_REGION_DTYPE, entry for entry next to network_bodies() (level 0) or network_groups() (1)"""
        return self._drainage_table(self._L.lbmdem_download_netflux_regions, NETFLUX_REGION_DTYPE)

    def netflux_profile(self):
        """(col, row), int64 [lx - 1] and [ly - 1]: the net mass through the section between rows x and x + 1 towards +x, and
        between columns y and y + 1 towards +y"""
        col, row = np.zeros(self.lx, np.int64), np.zeros(self.ly, np.int64)
        _chk(self._L.lbmdem_download_netflux_profile(self._h, _vp(col), _vp(row)))
        return col[:self.lx - 1].copy(), row[:self.ly - 1].copy()

    def write_netflux(self, directory=".", nFile=0, merge=-1, level=0):
        """netflux_links%.6i.dat, netflux_regions%.6i.dat, netflux_profile%.6i.dat and a line of netflux.data of the map and the
        populations as they are now"""
        _chk(self._L.lbmdem_write_netflux(self._h, os.fsencode(directory), int(nFile), int(merge), int(level)))

    def set_netflux_output(self, on=True, merge=-1, level=0):
        """run_scene writes the pore flux files at every DEM event, behind the network files"""
        _chk(self._L.lbmdem_set_netflux_output(self._h, 1 if on else 0, int(merge), int(level)))

    # network pressures: the pore network as a resistor network between an inlet and an outlet side (include/lbmdem_hip.h)
    def netsolve(self, frm, band, to, merge=-1, level=0, model=0, g=None, rtol=1e-8, max_iter=0, map=None):
        """pressures and flows of the pore network at `merge` (level 0: the bodies, 1: the groups) of the handle's map -- or of
        `map`, (lx, ly) ints as clearance() takes them -- with the regions within `band` nodes of the sides `frm` (SIDE_B | SIDE_T |
        SIDE_L | SIDE_R) held at p = 1 and those of `to` at p = 0: a Jacobi-preconditioned conjugate gradient to the relative
        residual `rtol`, at most `max_iter` iterations (0: the number of free regions, at most 100 000). model 0: the conductance of
        a link from its saddle (plane Poiseuille); model 1: `g`, one positive double per link of network_links(level). Runs
        network() first where its result at this merge is not there -> (dict of NETSOLVE_COUNTERS, dict of NETSOLVE_SUMS)"""
        c = np.zeros(len(NETSOLVE_COUNTERS), np.int64)
        sm = np.zeros(len(NETSOLVE_SUMS), np.float64)
        m = None
        if map is not None:
            m = np.ascontiguousarray(map, dtype=np.int32)
            if m.shape != (self.lx, self.ly):
                raise LbmDemError(-1, "netsolve: a map of shape (lx, ly)")
        gu = None if g is None else np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
        _chk(self._L.lbmdem_netsolve_compute(self._h, None if m is None else _vp(m), int(merge), int(level), int(frm), int(band), int(to),
                                             int(model), None if gu is None else _vp(gu), float(rtol), int(max_iter), _vp(c), _vp(sm)))
        counts = dict(zip(NETSOLVE_COUNTERS, (int(v) for v in c)))
        sums = dict(zip(NETSOLVE_SUMS, (float(v) for v in sm)))
        self._netsolve_last = (int(frm), int(to), sums["Q_in"])
        return counts, sums

    def netsolve_regions(self):
        """structured array of NETSOLVE_REGION_DTYPE, entry for entry next to network_bodies() (level 0) or network_groups() (1)"""
        return self._drainage_table(self._L.lbmdem_download_netsolve_regions, NETSOLVE_REGION_DTYPE)

    def netsolve_links(self):
        """structured array of NETSOLVE_LINK_DTYPE, entry for entry next to network_links(level) of the last netsolve()"""
        return self._drainage_table(self._L.lbmdem_download_netsolve_links, NETSOLVE_LINK_DTYPE)

    def netsolve_rounds(self):
        """the launches the iteration of the last netsolve() took: two per iteration enqueued, in whole batches"""
        r = C.c_int(0)
        _chk(self._L.lbmdem_netsolve_rounds(self._h, C.byref(r)))
        return r.value

    def netsolve_permeability(self):
        """Q_in * L / W of the last netsolve(): L the lattice's extent along the flow, W across it, in nodes; in units of the
        conductance model (model 0: node spacings squared at unit viscosity). Only for frm / to one pair of opposite sides."""
        last = getattr(self, "_netsolve_last", None)
        if last is None:
            raise ValueError("netsolve_permeability: no netsolve() has been made")
        frm, to, q_in = last
        if (frm, to) in ((SIDE_B, SIDE_T), (SIDE_T, SIDE_B)):
            return q_in * self.ly / self.lx
        if (frm, to) in ((SIDE_L, SIDE_R), (SIDE_R, SIDE_L)):
            return q_in * self.lx / self.ly
        raise ValueError("netsolve_permeability: frm and to must be one pair of opposite sides (%d, %d)" % (frm, to))

    def write_netsolve(self, directory=".", nFile=0, frm=SIDE_T, band=1, to=SIDE_B, merge=-1, level=0, rtol=1e-8, max_iter=0):
        """netsolve_regions%.6i.dat, netsolve_links%.6i.dat and a line of netsolve.data of the map as it is now (model 0)"""
        _chk(self._L.lbmdem_write_netsolve(self._h, os.fsencode(directory), int(nFile), int(merge), int(level), int(frm), int(band),
                                           int(to), float(rtol), int(max_iter)))

    def set_netsolve_output(self, on=True, frm=SIDE_T, band=1, to=SIDE_B, merge=-1, level=0, rtol=1e-8, max_iter=0):
        """run_scene writes the network pressure files at every DEM event, behind the pore flux files"""
        _chk(self._L.lbmdem_set_netsolve_output(self._h, 1 if on else 0, int(merge), int(level), int(frm), int(band), int(to),
                                                float(rtol), int(max_iter)))

    # coarse-grained fields: per cell of cw x ch nodes the sums of fluid, grains and contacts (include/lbmdem_hip.h)
    def coarse_fields(self, cw, ch):
        """-> (cells, outside, contacts_valid): cells a structured array of COARSE_DTYPE, shape (ncx, ncy); outside the grains
        whose centre lies off the lattice; contacts_valid 1 when the last sub-step was a table sub-step (else sum_z .. M22 are 0)"""
        count = C.c_long(0)
        info = np.zeros(2, np.int64)
        _chk(self._L.lbmdem_coarse_fields(self._h, int(cw), int(ch), None, 0, C.byref(count), _vp(info)))
        ncx, ncy = coarse_grid(self.lx, self.ly, cw, ch)
        cells = np.zeros((ncx, ncy), dtype=COARSE_DTYPE)
        _chk(self._L.lbmdem_coarse_fields(self._h, int(cw), int(ch), _vp(cells), cells.size, C.byref(count), _vp(info)))
        return cells, int(info[0]), int(info[1])

    def write_coarse(self, directory=".", nFile=0, cw=16, ch=16):
        """coarse%.6i.dat of the present state (write_coarse_files applied to coarse_fields)"""
        _chk(self._L.lbmdem_write_coarse(self._h, os.fsencode(directory), int(nFile), int(cw), int(ch)))

    def set_coarse_output(self, cw=0, ch=0):
        """run_scene writes coarse%.6i.dat with cells of cw x ch nodes at every DEM event, behind write_DEM / write_forces and
        the contact files; 0, 0 switches it off"""
        _chk(self._L.lbmdem_set_coarse_output(self._h, int(cw), int(ch)))

    # flow fields: composite velocity, vorticity, divergence, the collision's strain-rate moments, shear rate, dissipation
    # (include/lbmdem_hip.h)
    def flow_fields(self, mask=FLOW_ALL, device=False):
        """-> {name: (lx, ly) float64 array} of the fields `mask` selects (FLOW_UX .. FLOW_DISS), lattice units. device=True:
        torch.float64 tensors on the handle's GPU, filled by the kernel without a host copy on the handle's stream -- order
        through set_stream or sync()."""
        names = flow_plane_names(mask)
        if device:
            import torch
            out = torch.empty((len(names), self.lx, self.ly), dtype=torch.float64, device=f"cuda:{self.cfg.device}")
            self.flow_fields_into(mask, out)
            return {name: out[k] for k, name in enumerate(names)}
        count = C.c_long(0)
        out = np.zeros((len(names), self.lx, self.ly))
        _chk(self._L.lbmdem_flow_fields(self._h, int(mask), _vp(out), out.size, C.byref(count)))
        return {name: out[k] for k, name in enumerate(names)}

    def flow_fields_into(self, mask, tensor):
        """the planes of `mask` into a contiguous torch.float64 CUDA tensor of at least that many elements (no synchronisation)"""
        import torch
        if tensor.dtype != torch.float64 or not tensor.is_cuda or not tensor.is_contiguous():
            raise LbmDemError(-1, "flow_fields_into: a contiguous torch.float64 CUDA tensor")
        _chk(self._L.lbmdem_flow_fields_device(self._h, int(mask), C.c_void_p(tensor.data_ptr()), int(tensor.numel())))

    def flow_sums(self):
        """-> dict of FLOW_SUMS over the fluid nodes: n_fluid, sums of rho, kinetic energy, dissipation and enstrophy, maxima of
        u^2, the shear rate and |div| (lattice units; fixed order of additions, include/lbmdem_hip.h)"""
        out = np.zeros(8)
        _chk(self._L.lbmdem_flow_sums(self._h, _vp(out)))
        return dict(zip(FLOW_SUMS, (float(v) for v in out)))

    def write_flow(self, directory=".", nFile=0):
        """flow%.6i.vtk of the present state (write_flow_files applied to flow_fields; the byte image is made on the device)"""
        _chk(self._L.lbmdem_write_flow(self._h, os.fsencode(directory), int(nFile)))

    def set_flow_output(self, on=True):
        """run_scene writes flow%.6i.vtk at every VTK event, after the frame, and appends a line of flow_sums to flow.data at
        every DEM event"""
        _chk(self._L.lbmdem_set_flow_output(self._h, 1 if on else 0))

    # fluid tracers: massless particles carried by the composite velocity, one midpoint step per fluid step, on the device

    def set_tracers(self, xy, automatic=True):
        """n tracers at xy, (n, 2) node coordinates inside [0, lx - 1] x [0, ly - 1], replacing an earlier set; an empty array
        frees it. automatic: every fluid step advances them once, behind its force kernels; else only advance_tracers does."""
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        if xy.size == 0:
            xy = xy.reshape(0, 2)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise LbmDemError(-1, "set_tracers: positions of shape (n, 2)")
        _chk(self._L.lbmdem_tracer_set(self._h, len(xy), _vp(xy) if len(xy) else None, 1 if automatic else 0))

    def advance_tracers(self):
        """one advance in the present state, on the handle's stream (no synchronisation)"""
        _chk(self._L.lbmdem_tracer_advance(self._h))

    @property
    def tracers(self):
        """the positions, (n, 2)"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_tracer_download(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 2), np.float64)
        if n.value:
            _chk(self._L.lbmdem_tracer_download(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def tracer_sample(self):
        """(n, 3): the interpolated velocity U, V at every tracer and the owner of its nearest node"""
        n = C.c_long(0)
        _chk(self._L.lbmdem_tracer_sample(self._h, None, 0, C.byref(n)))
        out = np.empty((n.value, 3), np.float64)
        if n.value:
            _chk(self._L.lbmdem_tracer_sample(self._h, _vp(out), n.value, C.byref(n)))
        return out

    def tracer_stats(self):
        """{tracers, advances since set_tracers, hook_advances: those of them made by fluid steps}"""
        c = np.zeros(3, np.int64)
        _chk(self._L.lbmdem_tracer_stats(self._h, _vp(c)))
        return dict(zip(TRACER_COUNTERS, (int(v) for v in c)))

    def tracers_tensor(self):
        """the device buffer of the positions as a torch.float64 CUDA tensor (n, 2): a view, no copy -- an advance shows in it
        once the handle's stream has got there (sync()). Valid until the next set_tracers."""
        import torch
        p = C.c_void_p(None)
        _chk(self._L.lbmdem_tracer_device(self._h, C.byref(p)))
        n = self.tracer_stats()["tracers"]
        if not p.value or n == 0:
            return torch.empty((0, 2), dtype=torch.float64, device=f"cuda:{self.cfg.device}")
        return torch.as_tensor(_DeviceBlock(p.value, (n, 2)), device=f"cuda:{self.cfg.device}")

    def write_tracers(self, directory=".", nFile=0):
        """tracers%.6i.vtk of the present positions (write_tracers_files applied to tracers and tracer_sample)"""
        _chk(self._L.lbmdem_write_tracers(self._h, os.fsencode(directory), int(nFile)))

    def set_tracer_output(self, on=True):
        """run_scene writes tracers%.6i.vtk at every VTK event, after the frame and the flow file"""
        _chk(self._L.lbmdem_set_tracer_output(self._h, 1 if on else 0))

    # passive scalar: a dye field advected by the fluid's velocity and diffused, five populations per node, on the device

    def set_scalar(self, C_plane, tau_s=1.0, automatic=True):
        """the dye field from the concentration plane (lx, ly): w_k * C on the fluid nodes of the present map, replacing an
        earlier scalar; None removes it and frees its buffers. tau_s > 0.5 is the relaxation time: diffusivity (tau_s - 0.5) / 3
        in lattice units. automatic: every fluid step steps the field once, behind its force kernels; else only step_scalar."""
        if C_plane is None:
            _chk(self._L.lbmdem_scalar_set(self._h, None, 0.0, 0))
            return
        plane = np.ascontiguousarray(C_plane, dtype=np.float64)
        if plane.shape != (self.lx, self.ly):
            raise LbmDemError(-1, f"set_scalar: a plane of shape ({self.lx}, {self.ly})")
        _chk(self._L.lbmdem_scalar_set(self._h, _vp(plane), float(tau_s), 1 if automatic else 0))

    def step_scalar(self):
        """one step of the field in the present state, on the handle's stream (no synchronisation)"""
        _chk(self._L.lbmdem_scalar_step(self._h))

    @property
    def scalar(self):
        """the concentration plane (lx, ly), +0.0 where the scalar holds nothing"""
        out = np.empty((self.lx, self.ly), np.float64)
        _chk(self._L.lbmdem_scalar_download(self._h, _vp(out)))
        return out

    def scalar_state(self):
        """-> (g, was): the populations (lx, ly, 5) and the scalar's record of the fluid nodes (lx, ly) bool"""
        g = np.empty((self.lx, self.ly, 5), np.float64)
        was = np.empty((self.lx, self.ly), np.uint8)
        _chk(self._L.lbmdem_scalar_download_state(self._h, _vp(g), _vp(was)))
        return g, was.astype(bool)

    def scalar_tensor(self, refresh=True):
        """a concentration plane on the device as a torch.float64 CUDA tensor (lx, ly): a view, no copy. refresh writes the
        present field into it on the handle's stream (sync() before reading it); a step does not touch it. Valid until the next
        set_scalar."""
        import torch
        p = C.c_void_p(None)
        _chk(self._L.lbmdem_scalar_device(self._h, C.byref(p), 1 if refresh else 0))
        if not p.value:
            raise LbmDemError(-1, "scalar_tensor: no scalar is set (set_scalar first)")
        return torch.as_tensor(_DeviceBlock(p.value, (self.lx, self.ly)), device=f"cuda:{self.cfg.device}")

    def scalar_sums(self):
        """-> dict of SCALAR_SUMS over the nodes the scalar holds: their count, the sums of C and C * C (fixed order of additions,
        include/lbmdem_hip.h), the smallest and the largest C"""
        out = np.zeros(5)
        _chk(self._L.lbmdem_scalar_sums(self._h, _vp(out)))
        return dict(zip(SCALAR_SUMS, (float(v) for v in out)))

    def scalar_stats(self):
        """{present, steps since set_scalar, hook_steps: those of them made by fluid steps}"""
        c = np.zeros(3, np.int64)
        _chk(self._L.lbmdem_scalar_stats(self._h, _vp(c)))
        return dict(zip(SCALAR_COUNTERS, (int(v) for v in c)))

    def write_scalar(self, directory=".", nFile=0):
        """scalar%.6i.vtk of the present field (write_scalar_files applied to scalar)"""
        _chk(self._L.lbmdem_write_scalar(self._h, os.fsencode(directory), int(nFile)))

    def set_scalar_output(self, on=True):
        """run_scene writes scalar%.6i.vtk at every VTK event, after the frame, and appends a line of scalar_sums to scalar.data
        at every DEM event, while a scalar is set"""
        _chk(self._L.lbmdem_set_scalar_output(self._h, 1 if on else 0))

    # time-averaged flow statistics: per-node sums over the fluid steps of a window, accumulated on the device
    # (include/lbmdem_hip.h)
    def begin_mean(self, mask=MEAN_ALL, every=1):
        """opens a window with the accumulators of `mask` (MEAN_U .. MEAN_GRAIN), all zero, discarding an open one. every >= 1: the
        k-th fluid step from now on is sampled when k % every == 0, behind its force kernels; every == 0: only sample_mean."""
        _chk(self._L.lbmdem_mean_begin(self._h, int(mask), int(every)))

    def sample_mean(self):
        """one sample of the present state into the window, on the handle's stream"""
        _chk(self._L.lbmdem_mean_sample(self._h))

    def reset_mean(self):
        """zeroes the window; the mask, `every` and the phase of the cadence stay"""
        _chk(self._L.lbmdem_mean_reset(self._h))

    def end_mean(self):
        """closes the window and frees its memory"""
        _chk(self._L.lbmdem_mean_end(self._h))

    def mean_stats(self):
        """{present, mask, samples, hook_steps: the fluid steps the hook has counted, bytes the window holds}"""
        c = np.zeros(5, dtype=np.int64)
        _chk(self._L.lbmdem_mean_stats(self._h, _vp(c)))
        return dict(zip(MEAN_COUNTERS, (int(v) for v in c)))

    def mean_accumulators(self):
        """-> {name: (lx, ly) array}: the raw sums of the window's mask (float64, MEAN_PLANES) and n_fluid, n_grain (uint32)"""
        names = mean_plane_names(self.mean_stats()["mask"] or MEAN_ALL)
        planes = np.zeros((len(names), self.lx, self.ly))
        nf, ng = np.zeros((self.lx, self.ly), np.uint32), np.zeros((self.lx, self.ly), np.uint32)
        count = C.c_long(0)
        _chk(self._L.lbmdem_mean_download(self._h, _vp(planes), _vp(nf), _vp(ng), planes.size, C.byref(count)))
        out = {name: planes[k] for k, name in enumerate(names)}
        out.update(n_fluid=nf, n_grain=ng)
        return out

    def mean_fields(self, fmask=MEANF_ALL, device=False):
        """-> {name: (lx, ly) float64 array} of the derived fields `fmask` selects (MEANF_PHI .. MEANF_GUY), +0.0 where a node's
        count is 0. device=True: torch.float64 tensors on the handle's GPU, filled on the handle's stream without a host copy."""
        names = mean_field_names(fmask)
        if device:
            import torch
            out = torch.empty((len(names), self.lx, self.ly), dtype=torch.float64, device=f"cuda:{self.cfg.device}")
            self.mean_fields_into(fmask, out)
            return {name: out[k] for k, name in enumerate(names)}
        count = C.c_long(0)
        out = np.zeros((len(names), self.lx, self.ly))
        _chk(self._L.lbmdem_mean_fields(self._h, int(fmask), _vp(out), out.size, C.byref(count)))
        return {name: out[k] for k, name in enumerate(names)}

    def mean_fields_into(self, fmask, tensor):
        """the planes of `fmask` into a contiguous torch.float64 CUDA tensor of at least that many elements (no synchronisation)"""
        import torch
        if tensor.dtype != torch.float64 or not tensor.is_cuda or not tensor.is_contiguous():
            raise LbmDemError(-1, "mean_fields_into: a contiguous torch.float64 CUDA tensor")
        _chk(self._L.lbmdem_mean_fields_device(self._h, int(fmask), C.c_void_p(tensor.data_ptr()), int(tensor.numel())))

    def mean_profile(self):
        """-> (14, ly): per y the sum over x (x ascending, from +0.0) of each derived field and of n_fluid (MEAN_PROFILE_ROWS);
        divide by lx for the mean along x"""
        out = np.zeros((len(MEAN_PROFILE_ROWS), self.ly))
        _chk(self._L.lbmdem_mean_profile(self._h, _vp(out), out.size))
        return out

    def write_mean(self, directory=".", nFile=0):
        """mean%.6i.vtk and mean_profile%.6i.dat of the window (write_mean_files applied to mean_fields and mean_profile)"""
        _chk(self._L.lbmdem_write_mean(self._h, os.fsencode(directory), int(nFile)))

    def set_mean_output(self, mask=MEAN_ALL, every=1):
        """run_scene opens a window (mask, every) at its start, writes the two files at every VTK event and resets the window;
        mask 0 switches it off"""
        _chk(self._L.lbmdem_set_mean_output(self._h, int(mask), int(every)))

    def write_densities(self, directory=".", nFile=0):
        """write_densities (main.c:482-566): densities%.6i.vtk and pressure_base%.6i.dat, the text made on the device"""
        _chk(self._L.lbmdem_write_densities(self._h, os.fsencode(directory), int(nFile)))

    def densities_text(self):
        """bytes: the body of densities%.6i.vtk without its header lines -- all Pressure lines, then all velocity lines"""
        n = C.c_size_t(0)
        if self._L.lbmdem_download_densities_text(self._h, None, 0, C.byref(n)) == 0 or n.value == 0:
            _chk(self._L.lbmdem_download_densities_text(self._h, None, 0, C.byref(n)))   # (refused: say why)
            return b""
        out = np.empty(n.value, np.uint8)
        _chk(self._L.lbmdem_download_densities_text(self._h, _vp(out), n.value, C.byref(n)))
        return out[:n.value].tobytes()

    def set_densities_staging(self, nbytes):
        """the budget in bytes of the device and of the pinned staging buffer of write_densities; 0: the default (64 MiB)"""
        _chk(self._L.lbmdem_set_densities_staging(self._h, int(nbytes)))

    def densities_stats(self):
        """of the last write_densities / densities_text: (pressure bytes, velocity bytes, bands, nodes the device refused)"""
        c = np.zeros(4, np.int64)
        _chk(self._L.lbmdem_densities_stats(self._h, _vp(c)))
        return tuple(int(x) for x in c)

    def macro(self):
        rho, ux, uy = (np.zeros((self.lx, self.ly)) for _ in range(3))
        _chk(self._L.lbmdem_download_macro(self._h, _vp(rho), _vp(ux), _vp(uy)))
        return rho, ux, uy

    @property
    def kinematics(self):
        """(n, 9): x1 x2 x3 v1 v2 v3 a1 a2 a3"""
        out = np.zeros((self.n, 9))
        _chk(self._L.lbmdem_download_kinematics(self._h, _vp(out)))
        return out

    @kinematics.setter
    def kinematics(self, k):
        k = np.ascontiguousarray(k, dtype=np.float64)
        if k.shape != (self.n, 9):
            raise LbmDemError(-1, f"kinematics must have shape {(self.n, 9)}")
        _chk(self._L.lbmdem_upload_kinematics(self._h, _vp(k)))

    @property
    def fhf(self):
        out = np.zeros((self.n, 3))
        _chk(self._L.lbmdem_download_fhf(self._h, _vp(out)))
        return out

    @property
    def grain_pressure(self):
        out = np.zeros(self.n)
        _chk(self._L.lbmdem_download_grain_pressure(self._h, _vp(out)))
        return out

    def set_diagnostics(self, always=True):
        _chk(self._L.lbmdem_set_diagnostics(self._h, int(bool(always))))

    def grain_table(self):
        """(n, 30) in the reference's struct order (main.c:182-197)."""
        out = np.zeros((self.n, 30))
        _chk(self._L.lbmdem_download_grain_table(self._h, _vp(out)))
        return out

    def write_DEM(self, directory=".", nFile=0):
        """write_DEM (main.c:340-438): DEM%06d.dat + a line of stats.data.
        -> (KE, PE, SE, IFR, WF, INCE, TSLIP, TRW)"""
        e = np.zeros(8)
        _chk(self._L.lbmdem_write_dem(self._h, os.fsencode(directory), int(nFile), _vp(e)))
        return tuple(e)

    def write_forces(self, directory=".", nFile=0):
        """write_forces (main.c:440-478): DEM%06d.ps, grains + one line per overlapping pair."""
        _chk(self._L.lbmdem_write_forces(self._h, os.fsencode(directory), int(nFile)))

    def dem_stats(self):
        """the 22 numbers of the stats.data line of the last table sub-step (main.c:428-434), computed on the device, bit-equal
        to write_DEM's: time xfront xgrainmax height zmean energie_x energie_y energie_teta energie_cin N0..N5 energy_p SE WF IFR
        INCE TSLIP TRW"""
        out = np.zeros(22)
        _chk(self._L.lbmdem_dem_stats(self._h, _vp(out)))
        return out

    def set_async_dem(self, slots=2):
        """write_DEM / write_forces in the background: `slots` table slots (1..4) of device staging + pinned host memory; the
        writer thread and copy stream are those of set_async_output. 0 switches it off again (writes what is queued first).
        While on, run_scene queues its DEM events instead of writing them."""
        _chk(self._L.lbmdem_set_async_dem(self._h, int(slots)))

    def write_DEM_async(self, directory=".", nFile=0, forces=True):
        """write_DEM (+ write_forces) without the files' wait: two kernels and 22 numbers back, then copy, formatting, pair search
        and file I/O behind the run's back. Same files byte for byte once output_drain() has returned.
        -> (KE, PE, SE, IFR, WF, INCE, TSLIP, TRW), as write_DEM"""
        e = np.zeros(8)
        _chk(self._L.lbmdem_write_dem_async(self._h, os.fsencode(directory), int(nFile), int(bool(forces)), _vp(e)))
        return tuple(e)

    def output_stats_dem(self):
        """dict: DEM events queued / written / failed, calls that waited for a slot; ms the caller waited for a slot, the writer
        waited for copies, the writer spent formatting and in file I/O, the caller waited for the 22 numbers"""
        return self._output_stats(self._L.lbmdem_output_stats_dem, "ms_stats_wait")

    def write_vtk(self, directory=".", nFile=0):
        """write_vtk (main.c:237-338): five binary legacy-VTK files, byte-identical to the reference's."""
        _chk(self._L.lbmdem_write_vtk(self._h, os.fsencode(directory), int(nFile)))

    def set_async_output(self, frames=2):
        """Frames in the background: `frames` slots (1..4) of device staging + pinned host memory, a copy stream and one writer
        thread; 0 switches it off again (drains first). While on, run_scene queues its VTK frames instead of writing them."""
        _chk(self._L.lbmdem_set_async_output(self._h, int(frames)))

    def write_vtk_async(self, directory=".", nFile=0):
        """write_vtk without the wait: one snapshot kernel on the step stream, then copy and file I/O behind the run's back.
        Same files byte for byte once output_drain() has returned. Waits for a free slot when all are in flight."""
        _chk(self._L.lbmdem_write_vtk_async(self._h, os.fsencode(directory), int(nFile)))

    def output_drain(self):
        """returns when every queued frame is on disk; raises the writer's first failure since the last report"""
        _chk(self._L.lbmdem_output_drain(self._h))

    def output_stats(self):
        """dict: frames queued / written / failed, calls that waited for a slot; ms the caller waited for a slot, the writer
        waited for copies, the writer spent in file I/O, the caller spent in output_drain"""
        return self._output_stats(self._L.lbmdem_output_stats, "ms_drain")

    def vtk_image(self):
        """the frame image of the present state (the snapshot kernel alone, synchronously): bytes-like uint8[44 * lx * ly]"""
        out = np.zeros(44 * self.lx * self.ly, np.uint8)
        _chk(self._L.lbmdem_download_vtk_image(self._h, _vp(out)))
        return out

    def vtk_fields(self):
        nx = self.cfg.x_end - self.cfg.x_begin
        gp = np.zeros((self.ly, nx), np.float32); fp = np.zeros((self.ly, nx), np.float32)
        gv = np.zeros((self.ly, nx, 3), np.float32); ga = np.zeros((self.ly, nx, 3), np.float32)
        fv = np.zeros((self.ly, nx, 3), np.float32)
        _chk(self._L.lbmdem_download_vtk_fields(self._h, _vp(gp), _vp(gv), _vp(ga), _vp(fp), _vp(fv)))
        return gp, gv, ga, fp, fv

    def verlet(self):
        """-> (cumul[n], neighbours[npairs], wallflags[n]) in the reference's form."""
        npairs = C.c_int(0)
        cumul = np.zeros(self.n, np.int32)
        wf = np.zeros(self.n, np.int32)
        _chk(self._L.lbmdem_download_verlet(self._h, None, None, 0, C.byref(npairs), None))
        neigh = np.zeros(max(npairs.value, 1), np.int32)
        _chk(self._L.lbmdem_download_verlet(self._h, _vp(cumul), _vp(neigh), len(neigh), C.byref(npairs), _vp(wf)))
        return cumul, neigh[:npairs.value], wf

    def config(self) -> Config:
        out = Config()
        _chk(self._L.lbmdem_get_config(self._h, C.byref(out)))
        return out

    # ---- plumbing -------------------------------------------------------------------------------
    def set_lid(self, uw_h):
        """EXTENSION: the top plate's lid terms the reference has commented out (main.c:1129-1130); lattice units."""
        _chk(self._L.lbmdem_set_lid(self._h, float(uw_h)))

    def set_vibration(self, on=True):
        """The reference's shaken box (vib = 1, main.c:1700-1705): every renderScene / renderScene_dry moves the left and right
        walls by amp*sin(freq*t) first (freq, amp of the physics, clock from its t). Single-domain double-precision handles."""
        _chk(self._L.lbmdem_set_vibration(self._h, 1 if on else 0))

    @property
    def vibrating(self):
        return self._L.lbmdem_vibration(self._h) == 1

    def move_walls(self):
        """renderScene's wall motion alone (main.c:1700-1705), for runs driven phase by phase"""
        _chk(self._L.lbmdem_move_walls(self._h))

    def walls(self):
        """{t, Mgx, Mdx, Mby, Mhy} as the next sub-step finds them"""
        out = np.zeros(5)
        _chk(self._L.lbmdem_get_walls(self._h, _vp(out)))
        return dict(zip(("t", "Mgx", "Mdx", "Mby", "Mhy"), (float(v) for v in out)))

    # ---- device-side probes (include/lbmdem_hip.h: lbmdem_probe_*) ----------------------------------------------
    def probe_enable(self, every=1, capacity=1024, pressure_row=2, velocity_row=True, points=(), grain_extent=True):
        """Record the reference's uncalled field diagnostics on the device every `every`-th fluid step, right after
        forces_fluid: the pressure profile of row `pressure_row` (write_densities' pressure_base file, main.c:524-539; None
        or < 0: off), velocity_profile's row through grain 0 (main.c:1647-1676), `pressures` at the nodes `points` = [(x, y),
        ...] (main.c:1685-1691), xgrainmax and height (main.c:400-405). The ring holds `capacity` records; samples beyond that
        are dropped and counted until probe_read() empties it. Whole-lattice double-precision handles."""
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.int32).reshape(-1, 2))
        pc = ProbeConfig(int(every), int(capacity), -1 if pressure_row is None else int(pressure_row), int(bool(velocity_row)),
                         len(pts), pts.ctypes.data_as(C.POINTER(C.c_int)) if len(pts) else None, int(bool(grain_extent)))
        _chk(self._L.lbmdem_probe_enable(self._h, C.byref(pc)))

    def probe_disable(self):
        _chk(self._L.lbmdem_probe_disable(self._h))

    def probe_read(self):
        """The records since the last read, oldest first, as a dict of arrays -- step[n], time[n], clock[n] (a vibrating
        handle's t), pressure_row[n, lx], velocity_y[n], velocity_row[n, lx], point_pressure[n, npoints], xgrainmax[n],
        height[n]; fields switched off are absent -- plus `dropped`, the samples that found the ring full. Synchronises;
        empties the ring."""
        L = self._L
        count, dropped = C.c_long(0), C.c_long(0)
        _chk(L.lbmdem_probe_read(self._h, None, 0, C.byref(count), C.byref(dropped)))
        rec = int(L.lbmdem_probe_record_doubles(self._h))
        off = (C.c_long * 6)()
        _chk(L.lbmdem_probe_layout(self._h, off))
        buf = np.zeros((max(count.value, 1), rec))
        _chk(L.lbmdem_probe_read(self._h, _vp(buf), len(buf), C.byref(count), C.byref(dropped)))
        buf = buf[:count.value]
        out = dict(step=buf[:, 0].astype(np.int64), time=buf[:, 1].copy(), clock=buf[:, 2].copy(), dropped=int(dropped.value))
        if off[1] >= 0: out["pressure_row"] = buf[:, off[1]:off[1] + self.lx].copy()
        if off[2] >= 0: out["velocity_y"] = buf[:, off[2]].astype(np.int64)
        if off[3] >= 0: out["velocity_row"] = buf[:, off[3]:off[3] + self.lx].copy()
        if off[4] >= 0: out["point_pressure"] = buf[:, off[4]:(off[5] if off[5] >= 0 else rec)].copy()
        if off[5] >= 0:
            out["xgrainmax"], out["height"] = buf[:, off[5]].copy(), buf[:, off[5] + 1].copy()
        return out

    def set_force_mode(self, mode):
        _chk(self._L.lbmdem_set_force_mode(self._h, int(mode)))

    def set_dem_chain(self, max_substeps):
        """Longest run of ordinary sub-steps renderScene hands to ONE launch (< 2: one launch per sub-step)."""
        _chk(self._L.lbmdem_set_dem_chain(self._h, int(max_substeps)))

    def set_obst_update(self, on=True):
        """obst_construction writes only the nodes whose owner changes (default) / clears and repaints the map (False)"""
        _chk(self._L.lbmdem_set_obst_update(self._h, 1 if on else 0))

    def obst_stats(self):
        """(rasterisations that updated the map in place, rasterisations that cleared and repainted it)"""
        a, b = C.c_long(0), C.c_long(0)
        _chk(self._L.lbmdem_obst_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_change_mask(self, mode=1):
        """0: the fused kernel reads both obstacle maps everywhere; 1 (default): the previous map only in the rows the
        rasterisation marked as changed; 2: as 1, every use verified against the two maps (change_mask_stats()[1] == 0)"""
        _chk(self._L.lbmdem_set_change_mask(self._h, int(mode)))

    def change_mask_stats(self):
        """(fused launches that used the change bits, (row, window) pairs mode 2 found clear over differing maps)"""
        a, b = C.c_long(0), C.c_long(0)
        _chk(self._L.lbmdem_change_mask_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def measure_copy(self, nbytes=1200 * 1000 * 1000, reps=5):
        """GB/s (read + written) of a plain copy of `nbytes` on this handle's device: the box's yardstick"""
        g = C.c_double(0.0)
        _chk(self._L.lbmdem_measure_copy(self._h, int(nbytes), int(reps), C.byref(g)))
        return g.value

    def dem_chain_stats(self):
        """(launches, sub-steps covered, tile slots a launch needs resident, slots the census found; -1 = not taken)"""
        a, b, c, d = C.c_long(0), C.c_long(0), C.c_int(0), C.c_int(0)
        _chk(self._L.lbmdem_dem_chain_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def dem_chain_paints(self):
        """rasterisations done by the tail of a run of sub-steps instead of a launch of their own"""
        a = C.c_long(0)
        _chk(self._L.lbmdem_dem_chain_paints(self._h, C.byref(a)))
        return a.value

    def set_dem_tiles(self, mode):
        """1: the tiles of the multi-sub-step DEM kernel are patches of the packing (default); 0: 64 consecutive indices"""
        _chk(self._L.lbmdem_set_dem_tiles(self._h, int(mode)))

    def dem_chain_recoveries(self):
        """launches of the multi-sub-step kernel that gave up and were undone (the run went on one launch per sub-step)"""
        if not hasattr(self._L, "lbmdem_dem_chain_recoveries"):
            return 0
        a = C.c_long(0)
        _chk(self._L.lbmdem_dem_chain_recoveries(self._h, C.byref(a)))
        return a.value

    def debug_chain_giveup(self, launch):
        """experiment build: the launch of the multi-sub-step kernel with this number (from 0) gives up half way"""
        _chk(self._L.lbmdem_debug_chain_giveup(self._h, int(launch)))

    def force_stats(self):
        """(grains summed from the fused kernel's link table, grains gathered from the lattice) of the last
        forces_fluid call."""
        a, b = C.c_int(0), C.c_int(0)
        _chk(self._L.lbmdem_force_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_stream(self, hip_stream_ptr):
        """Enqueue on a caller-owned hipStream_t; 0/None = the HIP default stream."""
        _chk(self._L.lbmdem_set_stream(self._h, C.c_void_p(hip_stream_ptr or None)))

    def use_own_stream(self):
        _chk(self._L.lbmdem_use_own_stream(self._h))

    def sync(self):
        _chk(self._L.lbmdem_sync(self._h))

    def profile_enable(self, on=True):
        """HIP-event timing of the fused kernel; on = N > 1: every N-th launch only (two event records cost a step ~10 us)"""
        _chk(self._L.lbmdem_profile_enable(self._h, int(on)))

    def profile_read(self):
        ms, cnt = C.c_double(0), C.c_long(0)
        _chk(self._L.lbmdem_profile_read(self._h, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def halo_doubles(self):
        return int(self._L.lbmdem_halo_doubles(self._h))

    def halo_pack(self, side, dev_ptr):
        _chk(self._L.lbmdem_halo_pack(self._h, int(side), C.c_void_p(dev_ptr)))

    def halo_unpack(self, side, dev_ptr):
        _chk(self._L.lbmdem_halo_unpack(self._h, int(side), C.c_void_p(dev_ptr)))

    # ---- strips with distributed grains (include/lbmdem_hip.h: lbmdem_dist_*) --------------------------------------
    MSG_KIN, MSG_FHF, MSG_TABLES = 0, 1, 2

    def dist_default_margin(self):
        return int(self._L.lbmdem_dist_default_margin(self._h))

    def dist_enable(self, margin_rows=0):
        _chk(self._L.lbmdem_dist_enable(self._h, int(margin_rows)))

    def dist_message_doubles(self, kind):
        return int(self._L.lbmdem_dist_message_doubles(self._h, int(kind)))

    def dist_begin_period(self):
        _chk(self._L.lbmdem_dist_begin_period(self._h))

    def dist_pack(self, kind, side, dev_ptr):
        _chk(self._L.lbmdem_dist_pack(self._h, int(kind), int(side), C.c_void_p(dev_ptr)))

    def dist_unpack(self, kind, side, dev_ptr):
        _chk(self._L.lbmdem_dist_unpack(self._h, int(kind), int(side), C.c_void_p(dev_ptr)))

    def dist_pack2(self, kind, ptr_lo, ptr_hi):
        """both sides in one launch; None skips a side"""
        _chk(self._L.lbmdem_dist_pack2(self._h, int(kind), C.c_void_p(ptr_lo), C.c_void_p(ptr_hi)))

    def dist_unpack2(self, kind, ptr_lo, ptr_hi):
        _chk(self._L.lbmdem_dist_unpack2(self._h, int(kind), C.c_void_p(ptr_lo), C.c_void_p(ptr_hi)))

    def halo_pack2(self, ptr_lo, ptr_hi):
        _chk(self._L.lbmdem_halo_pack2(self._h, C.c_void_p(ptr_lo), C.c_void_p(ptr_hi)))

    def halo_unpack2(self, ptr_lo, ptr_hi):
        _chk(self._L.lbmdem_halo_unpack2(self._h, C.c_void_p(ptr_lo), C.c_void_p(ptr_hi)))

    # ---- drop-in outputs of a strip decomposition (include/lbmdem_hip.h) ----------------------------------
    def dist_export_carries(self):
        keys = np.zeros((3, 2), np.int64); vals = np.zeros(3); standing = np.zeros(3)
        _chk(self._L.lbmdem_dist_export_carries(self._h, _vp(keys), _vp(vals), _vp(standing)))
        return keys, vals, standing

    def dist_set_carries(self, carry3):
        c = np.ascontiguousarray(carry3, dtype=np.float64)
        _chk(self._L.lbmdem_dist_set_carries(self._h, _vp(c)))

    def path_info(self):
        """which size-dependent fast paths are active: dict(table, slots_per_direction, mincov, marching)"""
        v = (C.c_int * 4)()
        _chk(self._L.lbmdem_path_info(self._h, v))
        return dict(table=bool(v[0]), slots_per_direction=int(v[1]), mincov=bool(v[2]), marching=bool(v[3]))

    def fused_work_order(self):
        """how the fused kernel's launch is cut into work items: dict(levels, band_rows, chunk_rows, segment_rows [per level],
        level_rows [band rows cut at each level], items); levels == 0: uniform segments of segment_rows[0] rows"""
        v = (C.c_int * 12)()
        _chk(self._L.lbmdem_fused_work_order(self._h, v))
        nl = max(int(v[0]), 1)
        return dict(levels=int(v[0]), band_rows=int(v[1]), chunk_rows=int(v[2]), segment_rows=[int(v[3 + k]) for k in range(nl)],
                    level_rows=[int(v[7 + k]) for k in range(nl)], items=int(v[11]))

    def dist_export_owned(self):
        """-> (state12 [n][12], owned [n] uint8, carry_keys [3][2] int64, carry_vals [3]): what this rank contributes
        to the sub-step that feeds write_DEM (strips.merge_exports combines the ranks' exports)."""
        st = np.zeros((self.n, 12)); owned = np.zeros(self.n, np.uint8)
        keys = np.zeros((3, 2), np.int64); vals = np.zeros(3)
        _chk(self._L.lbmdem_dist_export_owned(self._h, _vp(st), _vp(owned), _vp(keys), _vp(vals)))
        return st, owned, keys, vals

    def dist_table_substep(self, state12_full, carry_vals, carry_has):
        """the root's sub-step on the full replica; afterwards grain_table / write_DEM / write_forces work here"""
        st = np.ascontiguousarray(state12_full, dtype=np.float64)
        cv = np.ascontiguousarray(carry_vals, dtype=np.float64); ch = np.ascontiguousarray(carry_has, dtype=np.int32)
        assert st.shape == (self.n, 12)
        _chk(self._L.lbmdem_dist_table_substep(self._h, _vp(st), _vp(cv), _vp(ch)))

    def vtk_place_owned(self, fields11):
        """this strip's columns of the five write_vtk fields into a zero-initialised float32 array of 11 * lx * ly"""
        assert fields11.dtype == np.float32 and fields11.size == 11 * self.lx * self.ly and fields11.flags.c_contiguous
        _chk(self._L.lbmdem_vtk_place_owned(self._h, _vp(fields11)))

    def dist_set_poison(self, on=True):
        _chk(self._L.lbmdem_dist_set_poison(self._h, 1 if on else 0))

    def fhf_export(self, dev_ptr):
        _chk(self._L.lbmdem_fhf_export(self._h, C.c_void_p(dev_ptr)))

    def fhf_import(self, dev_ptr):
        _chk(self._L.lbmdem_fhf_import(self._h, C.c_void_p(dev_ptr)))

    def fhf_device(self):
        a, b = C.c_void_p(), C.c_void_p()
        _chk(self._L.lbmdem_fhf_device(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value
