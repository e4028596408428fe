"""CPU: the extension of a checkpoint file (lbmdem_set_checkpoint_contents: "LBMXTRA1" and its five sections behind f, the
trailer "LBMCKSM2") as lbmdem_checkpoint_verify and lbmdem_checkpoint_contents read it, on files built in numpy from the layout
include/lbmdem_hip.h documents. No GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

from test_checkpoint_digest import digest_numpy

PLAIN = ("header", "r", "kin", "fhf", "gp", "offsets", "nbr", "wallflags", "obst", "f")
EXTRA = ("extras", "tracers", "scalar_g", "scalar_was", "mean_cnt", "mean_S")
N, NNBR, LX, LY = 7, 6, 20, 17
PLANE = LX * ((LY + 15) // 16 * 16)
MEAN_BIT_PLANES = (2, 3, 2, 2, 2)


def plain_parts(pkg):
    """the header (lbmdem_checkpoint.hip's CkptHeader, as test_checkpoint_digest.py restates it) and nine sections of zeros"""

    class Header(C.Structure):
        _fields_ = [("magic", C.c_char * 8), ("lid6", C.c_double), ("layout", C.c_int), ("force_mode", C.c_int),
                    ("diag_always", C.c_int), ("has_carry", C.c_int), ("carry", C.c_double * 3), ("cfg", pkg.Config),
                    ("nbsteps", C.c_long), ("verlet_ok", C.c_int), ("nnbr", C.c_int), ("plane", C.c_long),
                    ("has_dist", C.c_int), ("vib", C.c_int)]

    H = Header()
    H.magic, H.layout, H.has_carry, H.verlet_ok, H.nnbr = b"LBMDEMC5", 1, 1, 1, NNBR
    H.cfg = pkg.derive(LX, LY, np.full(N, 0.5e-3))
    H.nbsteps, H.plane = 60, PLANE
    lengths = [8 * N, 72 * N, 24 * N, 8 * N, 4 * (N + 1), 4 * NNBR, N, 4 * PLANE, 72 * PLANE]
    return [bytes(H)] + [b"\0" * nb for nb in lengths]


def extra_parts(mask=7, ntr=3, mean_mask=5, samples=4):
    """the extension header of 120 bytes and the five sections, those the mask does not name empty"""
    rng = np.random.default_rng(mask)
    nsel = sum(c for b, c in enumerate(MEAN_BIT_PLANES) if mean_mask >> b & 1)
    tr = (ntr, 1, 11, 9) if mask & 1 else (0, 0, 0, 0)
    sc = (0.8, 1, 10, 10) if mask & 2 else (0., 0, 0, 0)
    mn = (mean_mask, 3, nsel, samples, 10) if mask & 4 else (0, 0, 0, 0, 0)
    head = b"LBMXTRA1" + struct.pack("<iiq", mask, 0, PLANE) + struct.pack("<qiiqq", tr[0], tr[1], 0, tr[2], tr[3]) + \
        struct.pack("<diiqq", sc[0], sc[1], 0, sc[2], sc[3]) + struct.pack("<iiiiqq", mn[0], mn[1], mn[2], 0, mn[3], mn[4])
    assert len(head) == 120
    xy = rng.uniform(0, (LX - 1, LY - 1), (ntr, 2)).tobytes() if mask & 1 else b""
    g = rng.standard_normal(5 * PLANE).tobytes() if mask & 2 else b""
    was = rng.integers(0, 2, PLANE, dtype=np.uint8).tobytes() if mask & 2 else b""
    cnt = rng.integers(0, samples + 1, 2 * PLANE, dtype=np.uint32).tobytes() if mask & 4 else b""
    S = rng.standard_normal(nsel * PLANE).tobytes() if mask & 4 else b""
    return [head, xy, g, was, cnt, S]


def trailer(magic, parts):
    out = magic + struct.pack("<ii", len(parts), 0)
    for p in parts:
        out += struct.pack("<QQQ", len(p), *(digest_numpy(p) if p else (0, 0)))
    return out


def extended_file(pkg, **kw):
    parts = plain_parts(pkg) + extra_parts(**kw)
    return b"".join(parts) + trailer(b"LBMCKSM2", parts), parts


def test_verify_and_contents_of_a_file_made_without_a_gpu(pkg, tmp_path):
    data, parts = extended_file(pkg)
    assert len(trailer(b"LBMCKSM2", parts)) == 16 + 24 * 16
    p = tmp_path / "made.ckpt"
    p.write_bytes(data)
    assert pkg.LbmDem.checkpoint_verify(str(p)) is True
    assert pkg.LbmDem.checkpoint_contents(str(p)) == dict(mask=7, tracers=3, scalar_steps=10, mean_mask=5, mean_samples=4)
    # the same without a trailer: the synchronous save's file
    body = b"".join(parts)
    p.write_bytes(body)
    assert pkg.LbmDem.checkpoint_verify(str(p)) is False
    assert pkg.LbmDem.checkpoint_contents(str(p))["mask"] == 7


@pytest.mark.parametrize("mask", [1, 2, 4, 5])
def test_a_subset_has_empty_sections_with_zero_digests(pkg, tmp_path, mask):
    data, parts = extended_file(pkg, mask=mask, ntr=1, mean_mask=1, samples=2)
    assert [len(q) > 0 for q in parts[11:]] == [bool(mask & 1), bool(mask & 2), bool(mask & 2), bool(mask & 4), bool(mask & 4)]
    p = tmp_path / "subset.ckpt"
    p.write_bytes(data)
    assert pkg.LbmDem.checkpoint_verify(str(p)) is True
    got = pkg.LbmDem.checkpoint_contents(str(p))
    assert got == dict(mask=mask, tracers=mask & 1, scalar_steps=10 if mask & 2 else 0, mean_mask=1 if mask & 4 else 0,
                       mean_samples=2 if mask & 4 else 0)


def test_a_flipped_byte_names_its_section(pkg, tmp_path):
    data, parts = extended_file(pkg)
    p = tmp_path / "flipped.ckpt"
    at = sum(len(q) for q in parts[:10])
    for name, part in zip(EXTRA, parts[10:]):
        # (the extension header's first byte is its magic, its last one a counter: two different ways to fail, one name)
        for where in (at, at + len(part) // 2, at + len(part) - 1):
            bad = bytearray(data)
            bad[where] ^= 0x10
            p.write_bytes(bytes(bad))
            with pytest.raises(pkg.LbmDemError) as e:
                pkg.LbmDem.checkpoint_verify(str(p))
            assert e.value.code == -1 and f"section '{name}'" in str(e.value), (name, where, str(e.value))
        at += len(part)
    assert at + 16 + 24 * 16 == len(data)
    # ... and the ten sections in front of it still do
    bad = bytearray(data)
    bad[len(parts[0]) + 3] ^= 1
    p.write_bytes(bytes(bad))
    with pytest.raises(pkg.LbmDemError, match="section 'r'"):
        pkg.LbmDem.checkpoint_verify(str(p))


def test_cut_files_are_refused(pkg, tmp_path):
    data, parts = extended_file(pkg)
    p = tmp_path / "cut.ckpt"
    plain = sum(len(q) for q in parts[:10])
    body = sum(len(q) for q in parts)
    for keep in (plain + 5, plain + 60, plain + 120 + 7, plain + 120 + len(parts[11]) + 5 * 8 * PLANE // 2, body - 1):
        p.write_bytes(data[:keep])                      # inside the extension: its header, its sections
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.LbmDem.checkpoint_verify(str(p))
        assert e.value.code == -1 and ("extension" in str(e.value) or "shorter" in str(e.value)), (keep, str(e.value))
    p.write_bytes(data[:plain + 3])                     # "LBM": both magics begin so, and it is read as a trailer cut short, as ever
    with pytest.raises(pkg.LbmDemError, match="trailer"):
        pkg.LbmDem.checkpoint_verify(str(p))
    for keep in (body + 5, body + 8, body + 40, len(data) - 1):
        p.write_bytes(data[:keep])                      # inside the trailer
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.LbmDem.checkpoint_verify(str(p))
        assert "trailer" in str(e.value), (keep, str(e.value))
    p.write_bytes(data + b"\0")                         # something behind the trailer: not this format
    with pytest.raises(pkg.LbmDemError):
        pkg.LbmDem.checkpoint_verify(str(p))
    p.write_bytes(data[:plain + 60])
    with pytest.raises(pkg.LbmDemError, match="extension"):
        pkg.LbmDem.checkpoint_contents(str(p))


def test_a_trailer_must_cover_what_the_file_holds(pkg, tmp_path):
    """the old trailer behind an extension, and the new one without an extension: neither is a file this library writes"""
    parts = plain_parts(pkg) + extra_parts()
    p = tmp_path / "mixed.ckpt"
    p.write_bytes(b"".join(parts) + trailer(b"LBMCKSM1", parts[:10]))
    with pytest.raises(pkg.LbmDemError):
        pkg.LbmDem.checkpoint_verify(str(p))
    p.write_bytes(b"".join(parts[:10]) + trailer(b"LBMCKSM2", parts[:10] + [b""] * 6))
    with pytest.raises(pkg.LbmDemError, match="extras"):
        pkg.LbmDem.checkpoint_verify(str(p))


@pytest.mark.parametrize("what", ["mask", "plane", "count", "tau", "nsel", "negative"])
def test_implausible_extension_headers_are_refused(pkg, tmp_path, what):
    parts = plain_parts(pkg) + extra_parts()
    head = bytearray(parts[10])
    edit = dict(mask=(8, "<i", 15), plane=(16, "<q", PLANE + 16), count=(24, "<q", 1 << 40), tau=(56, "<d", 0.5),
                nsel=(96, "<i", 5), negative=(104, "<q", -1))[what]
    struct.pack_into(edit[1], head, edit[0], edit[2])
    parts[10] = bytes(head)
    p = tmp_path / "implausible.ckpt"
    p.write_bytes(b"".join(parts) + trailer(b"LBMCKSM2", parts))     # (the digests match: the header itself is at fault)
    with pytest.raises(pkg.LbmDemError, match="extras"):
        pkg.LbmDem.checkpoint_verify(str(p))
    with pytest.raises(pkg.LbmDemError, match="extension"):
        pkg.LbmDem.checkpoint_contents(str(p))


def test_a_plain_file_reports_no_contents(pkg, tmp_path):
    parts = plain_parts(pkg)
    p = tmp_path / "plain.ckpt"
    zero = dict(mask=0, tracers=0, scalar_steps=0, mean_mask=0, mean_samples=0)
    p.write_bytes(b"".join(parts))
    assert pkg.LbmDem.checkpoint_contents(str(p)) == zero and pkg.LbmDem.checkpoint_verify(str(p)) is False
    p.write_bytes(b"".join(parts) + trailer(b"LBMCKSM1", parts))
    assert pkg.LbmDem.checkpoint_contents(str(p)) == zero and pkg.LbmDem.checkpoint_verify(str(p)) is True
    p.write_bytes(b"no checkpoint" * 100)
    with pytest.raises(pkg.LbmDemError, match="not a checkpoint"):
        pkg.LbmDem.checkpoint_contents(str(p))
    with pytest.raises(pkg.LbmDemError):
        pkg.LbmDem.checkpoint_contents(str(tmp_path / "missing.ckpt"))
    assert (pkg.CKPT_TRACERS, pkg.CKPT_SCALAR, pkg.CKPT_MEAN, pkg.CKPT_ALL) == (1, 2, 4, 7)
