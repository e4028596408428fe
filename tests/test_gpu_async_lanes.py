"""GPU: the three kinds of background job (VTK frames, DEM tables, checkpoints) on ONE handle -- they share the writer thread, the
copy stream and the queue, and each has its own slots and counters. The 65 x 17 floor row of test_gpu_async_checkpoint.py (5
grains, diagnostics always on): the smallest case the suite trusts for all three snapshot kernels. All comparisons are exact; the
synchronous writers run first, on the same handle at the same state (they only read it)."""
import pytest

from test_gpu_async_checkpoint import check_async_file, floor_row, no_tmp_files
from test_gpu_async_dem import dem_names, stats_lines
from test_gpu_async_output import same_dirs, vtk_names

pytestmark = pytest.mark.gpu

ZEROS = dict(queued=0, written=0, failed=0, slot_waits=0, ms_slot_wait=0.0, ms_copy_wait=0.0, ms_io=0.0)


def floor_sim(pkg, tmp_path):
    lx, ly, r, x1, x2 = floor_row(65, 17)
    assert len(r) == 5
    sim = pkg.LbmDem(lx, ly, r, x1, x2)
    sim.set_diagnostics(True)
    sim.renderScene(25)
    ds, da = tmp_path / "sync", tmp_path / "async"
    ds.mkdir(); da.mkdir()
    return sim, ds, da


def counts(st):
    return st["queued"], st["written"], st["failed"]


def test_the_three_kinds_share_one_queue_in_call_order(pkg, tmp_path):
    sim, ds, da = floor_sim(pkg, tmp_path)
    for k in range(3):
        sim.write_DEM(str(ds), k); sim.write_forces(str(ds), k)
    for k in range(2):
        sim.write_vtk(str(ds), k)
    sim.checkpoint_save(str(tmp_path / "A.sync"))
    sim.set_async_output(1); sim.set_async_dem(1); sim.set_async_checkpoint(1)
    # one slot per kind, no step in between: the second frame and the later tables wait for the writer
    sim.write_DEM_async(str(da), 0)
    sim.write_vtk_async(str(da), 0)
    sim.checkpoint_save_async(str(tmp_path / "A.async"))
    sim.write_DEM_async(str(da), 1)
    sim.write_vtk_async(str(da), 1)
    sim.write_DEM_async(str(da), 2)
    sim.renderScene(12)              # nothing stepped here may reach a file
    sim.output_drain()
    lines = stats_lines(da)
    assert len(lines) == 3 and lines == stats_lines(ds)
    same_dirs(ds, da, vtk_names(0) + vtk_names(1) + dem_names(0, 1, 2))
    check_async_file(str(tmp_path / "A.async"), str(tmp_path / "A.sync"), sim)
    no_tmp_files(tmp_path)
    frames, tables, ckpts = sim.output_stats(), sim.output_stats_dem(), sim.output_stats_checkpoint()
    print("frames", frames, "\ntables", tables, "\ncheckpoints", ckpts)
    assert counts(frames) == (2, 2, 0) and counts(tables) == (3, 3, 0) and counts(ckpts) == (1, 1, 0)
    assert tables["slot_waits"] >= 1 and tables["ms_slot_wait"] > 0.0
    sim.close()


def test_one_kind_switched_off_with_the_others_in_flight(pkg, tmp_path):
    sim, ds, da = floor_sim(pkg, tmp_path)
    for k in range(2):
        sim.write_DEM(str(ds), k); sim.write_forces(str(ds), k)
    sim.write_vtk(str(ds), 0)
    sim.checkpoint_save(str(tmp_path / "A.sync"))
    sim.set_async_output(1); sim.set_async_dem(1); sim.set_async_checkpoint(1)
    sim.write_vtk_async(str(da), 0)
    sim.output_drain()
    assert counts(sim.output_stats()) == (1, 1, 0)
    sim.write_DEM_async(str(da), 0)
    sim.checkpoint_save_async(str(tmp_path / "A.async"))
    sim.set_async_output(0)          # the writer is shared: what the other two have queued is on disk when this returns
    assert sorted(p.name for p in da.iterdir()) == sorted(vtk_names(0) + dem_names(0))
    for n in dem_names(0)[:2]:
        assert (da / n).read_bytes() == (ds / n).read_bytes(), n
    assert stats_lines(da) == stats_lines(ds)[:1]
    check_async_file(str(tmp_path / "A.async"), str(tmp_path / "A.sync"), sim)
    no_tmp_files(tmp_path)
    tables, ckpts = sim.output_stats_dem(), sim.output_stats_checkpoint()
    assert counts(tables) == (1, 1, 0) and counts(ckpts) == (1, 1, 0)          # another kind's setter leaves them alone
    assert tables["ms_io"] > 0.0 and ckpts["ms_io"] > 0.0 and ckpts["ms_hold"] > 0.0
    assert sim.output_stats() == dict(ZEROS, ms_drain=0.0)
    sim.set_async_dem(0); sim.set_async_checkpoint(0)                           # the last kind off: writer and copy stream go
    assert sim.output_stats_dem() == dict(ZEROS, ms_stats_wait=0.0)
    assert sim.output_stats_checkpoint() == dict(ZEROS, ms_hold=0.0)
    with pytest.raises(pkg.LbmDemError):
        sim.write_vtk_async(str(da), 1)
    sim.set_async_dem(1)                                                        # ... and come back
    sim.write_DEM_async(str(da), 1)
    sim.output_drain()
    same_dirs(ds, da, vtk_names(0) + dem_names(0, 1))
    assert counts(sim.output_stats_dem()) == (1, 1, 0)
    no_tmp_files(tmp_path)
    sim.close()
