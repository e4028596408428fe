"""GPU: what the read-only exports and the setters that go with them answer when they cannot serve a handle -- a strip of a
decomposition, a handle with distributed grains, the float library, a directory that does not exist -- each as the complete
error text of the library that refused.

lbmdem_write_vtk_async looks for its slots before it looks at the handle, and neither a strip nor a handle with distributed
grains can have slots (lbmdem_set_async_output refuses the one, lbmdem_dist_enable a handle that has them): there its answer
is that frames in the background are off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LX, LY = 64, 48
R = np.array([0.6e-3, 0.7e-3, 0.5e-3])
X1 = np.array([1.5e-3, 3.4e-3, 5.0e-3])
X2 = np.array([1.2e-3, 2.6e-3, 1.4e-3])

WHOLE = (" needs the whole lattice and all grains on this handle (not a strip of a decomposition, no distributed grains)")
SP = " is not available in the single-precision build of the library"
VTK_THERE = ": use lbmdem_comm_write_vtk there"
CKPT_THERE = ": there every rank saves its own file with lbmdem_checkpoint_save"
ASYNC_OFF = "lbmdem_write_vtk_async: async output is off (lbmdem_set_async_output)"
LINKS, CONTACTS, COARSE, FLOW = ("the boundary-link export", "the contact network export", "the coarse-grained fields export",
                                 "the flow fields export")


def into(sim):
    import torch
    sim.flow_fields_into(1, torch.empty(LX * LY, dtype=torch.float64, device=f"cuda:{sim.cfg.device}"))


# method, the call, the text on a strip and on a handle with distributed grains, the float library's noun (None: it serves)
TABLE = [
    ("geometry_stats", lambda s: s.geometry_stats(), "lbmdem_geometry_stats" + WHOLE, LINKS),
    ("download_act", lambda s: s.download_act(), "lbmdem_download_act" + WHOLE, LINKS),
    ("download_links", lambda s: s.download_links(), "lbmdem_download_links" + WHOLE, LINKS),
    ("download_geometry_obst", lambda s: s.download_geometry_obst(), "lbmdem_download_geometry_obst" + WHOLE, LINKS),
    ("write_obst", lambda s: s.write_obst("."), "lbmdem_download_geometry_obst" + WHOLE, LINKS),
    ("contact_stats", lambda s: s.contact_stats(), "lbmdem_contact_stats" + WHOLE, CONTACTS),
    ("download_contacts", lambda s: s.download_contacts(), "lbmdem_download_contacts" + WHOLE, CONTACTS),
    ("write_contacts", lambda s: s.write_contacts(".", 0), "lbmdem_download_contacts" + WHOLE, CONTACTS),
    ("set_contacts_output", lambda s: s.set_contacts_output(True), "lbmdem_set_contacts_output" + WHOLE, CONTACTS),
    ("coarse_fields", lambda s: s.coarse_fields(16, 16), "lbmdem_coarse_fields" + WHOLE, COARSE),
    ("write_coarse", lambda s: s.write_coarse(".", 0, 16, 16), "lbmdem_coarse_fields" + WHOLE, COARSE),
    ("set_coarse_output", lambda s: s.set_coarse_output(16, 16), "lbmdem_set_coarse_output" + WHOLE, COARSE),
    ("flow_fields", lambda s: s.flow_fields(1), "lbmdem_flow_fields" + WHOLE, FLOW),
    ("flow_fields_into", into, "lbmdem_flow_fields_device" + WHOLE, FLOW),
    ("flow_sums", lambda s: s.flow_sums(), "lbmdem_flow_sums" + WHOLE, FLOW),
    ("write_flow", lambda s: s.write_flow(".", 0), "lbmdem_write_flow" + WHOLE, FLOW),
    ("set_flow_output", lambda s: s.set_flow_output(True), "lbmdem_set_flow_output" + WHOLE, FLOW),
    ("write_densities", lambda s: s.write_densities(".", 0), "lbmdem_write_densities" + WHOLE, "write_densities"),
    ("densities_text", lambda s: s.densities_text(), "lbmdem_download_densities_text" + WHOLE, "write_densities"),
    ("write_vtk_async", lambda s: s.write_vtk_async(".", 0), ASYNC_OFF, None),
    ("set_async_output", lambda s: s.set_async_output(1), "lbmdem_set_async_output" + WHOLE + VTK_THERE, None),
    ("set_checkpoint_every", lambda s: s.set_checkpoint_every(100, "refused.ckpt"),
     "lbmdem_set_checkpoint_every" + WHOLE + CKPT_THERE, "checkpointing"),
]
IDS = [t[0] for t in TABLE]


@pytest.fixture(scope="module")
def handles(pkg):
    strip = pkg.LbmDem(LX, LY, R, X1, X2, strip=(LX // 2, LX), halo=12)
    dist = pkg.LbmDem(LX, LY, R, X1, X2)
    dist.dist_enable()
    f32 = pkg.LbmDem(LX, LY, R, X1, X2, precision="f32")
    yield {"strip": strip, "dist": dist, "f32": f32}
    for sim in (strip, dist, f32):
        sim.close()


def refusal(pkg, sim, call):
    """the complete text of the library the handle belongs to"""
    with pytest.raises(pkg.LbmDemError) as e:
        call(sim)
    assert e.value.code == -1, e.value
    return sim._L.lbmdem_last_error().decode()


@pytest.mark.parametrize("name,call,text,noun", TABLE, ids=IDS)
def test_strip_and_distributed_grains(pkg, handles, name, call, text, noun):
    assert refusal(pkg, handles["strip"], call) == text
    assert refusal(pkg, handles["dist"], call) == text


@pytest.mark.parametrize("name,call,text,noun", [t for t in TABLE if t[3]], ids=[t[0] for t in TABLE if t[3]])
def test_float_library(pkg, handles, name, call, text, noun):
    assert refusal(pkg, handles["f32"], call) == noun + SP


def test_directory_that_does_not_exist(pkg, tmp_path):
    missing = str(tmp_path / "missing")
    sim = pkg.LbmDem(LX, LY, R, X1, X2)
    assert refusal(pkg, sim, lambda s: s.write_obst(missing)) == f"cannot open '{missing}/obst_LB.dat' for writing"
    sim.set_diagnostics(True)
    sim.run_dem(1)   # a table sub-step: there is a contact network to write
    for call, name in ((lambda s: s.write_contacts(missing, 0), "contacts000000.dat"),
                       (lambda s: s.write_coarse(missing, 0, 16, 16), "coarse000000.dat"),
                       (lambda s: s.write_flow(missing, 0), "flow000000.vtk"),
                       (lambda s: s.write_densities(missing, 0), "densities000000.vtk")):
        assert refusal(pkg, sim, call) == f"cannot open '{missing}/{name}' for writing"
    sim.set_async_output(1)   # the writer thread opens the frame's files: its failure comes back with the drain
    sim.write_vtk_async(missing, 0)
    assert refusal(pkg, sim, lambda s: s.output_drain()) == \
        f"background frame writer: cannot open '{missing}/grain_pressure_000000.vtk' for writing"
    sim.set_async_output(0)
    sim.close()
