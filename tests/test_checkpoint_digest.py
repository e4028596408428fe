"""CPU: the digest of a checkpoint section (lbmdem_checkpoint_digest, the one routine the background writer and
lbmdem_checkpoint_verify use) against a numpy restatement in wrapping uint64 arithmetic, and the verifier's answers on files that
are no checkpoints. No GPU."""
import numpy as np
import pytest


def digest_numpy(data: bytes):
    """W = ceil(B / 8) little-endian uint64 words, the last zero-padded; S1 = sum w_i, S2 = sum (i + 1) w_i, both mod 2^64"""
    pad = (-len(data)) % 8
    w = np.frombuffer(data + b"\0" * pad, dtype="<u8")
    with np.errstate(over="ignore"):
        s1 = np.add.reduce(w, dtype=np.uint64) if w.size else np.uint64(0)
        idx = np.arange(1, w.size + 1, dtype=np.uint64)
        s2 = np.add.reduce(idx * w, dtype=np.uint64) if w.size else np.uint64(0)
    return int(s1), int(s2)


def digest_python(data: bytes):
    """the same once more in Python's unbounded integers (keeps the numpy restatement honest about wrapping)"""
    data = data + b"\0" * ((-len(data)) % 8)
    s1 = s2 = 0
    for i in range(len(data) // 8):
        w = int.from_bytes(data[8 * i:8 * i + 8], "little")
        s1 += w
        s2 += (i + 1) * w
    return s1 % 2 ** 64, s2 % 2 ** 64


@pytest.mark.parametrize("nbytes", [0, 1, 7, 8, 9, 4099, 300 * 1024 + 5])
def test_digest_equals_the_numpy_restatement(pkg, nbytes):
    data = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8).tobytes()
    got = pkg.LbmDem.checkpoint_digest(data)
    assert got == digest_numpy(data)
    if nbytes <= 4099:
        assert got == digest_python(data)
    if nbytes == 0:
        assert got == (0, 0)


def test_digest_wraps_and_weighs_by_position(pkg):
    ones = b"\xff" * 64                                   # eight words of 2^64 - 1: both sums wrap
    assert pkg.LbmDem.checkpoint_digest(ones) == digest_python(ones) == ((-8) % 2 ** 64, (-36) % 2 ** 64)
    a, b = b"\1" + b"\0" * 15, b"\0" * 8 + b"\1" + b"\0" * 7   # the same word in another place: S1 equal, S2 not
    da, db = pkg.LbmDem.checkpoint_digest(a), pkg.LbmDem.checkpoint_digest(b)
    assert da == (1, 1) and db == (1, 2)
    assert pkg.LbmDem.checkpoint_digest(b"\0\0\0\x80") == (0x80000000, 0x80000000)   # a short last word is zero-padded
    assert pkg.LbmDem.checkpoint_digest(np.arange(5, dtype=np.uint8)) == digest_python(bytes(range(5)))


def test_verify_refuses_what_is_no_checkpoint(pkg, tmp_path):
    with pytest.raises(pkg.LbmDemError) as e:
        pkg.LbmDem.checkpoint_verify(str(tmp_path / "missing.ckpt"))
    assert e.value.code == -1
    p = tmp_path / "text.ckpt"
    p.write_bytes(b"not a checkpoint at all" * 40)
    with pytest.raises(pkg.LbmDemError) as e:
        pkg.LbmDem.checkpoint_verify(str(p))
    assert e.value.code == -1 and "not a checkpoint" in str(e.value)


def synthetic_checkpoint(pkg, n=7, nnbr=6, lx=20, ly=17, with_trailer=True):
    """a file with the LBMDEMC5 header (lbmdem_checkpoint.hip's CkptHeader, restated here), sections of random bytes of the
    lengths the header implies, and the digest trailer computed with numpy: what the verifier reads, made without a GPU"""
    import ctypes as C

    class Header(C.Structure):
        _fields_ = [("magic", C.c_char * 8), ("lid6", C.c_double), ("layout", C.c_int), ("force_mode", C.c_int),
                    ("diag_always", C.c_int), ("has_carry", C.c_int), ("carry", C.c_double * 3), ("cfg", pkg.Config),
                    ("nbsteps", C.c_long), ("verlet_ok", C.c_int), ("nnbr", C.c_int), ("plane", C.c_long),
                    ("has_dist", C.c_int), ("vib", C.c_int)]

    r = np.full(n, 0.5e-3)
    H = Header()
    H.magic, H.layout, H.has_carry, H.verlet_ok, H.nnbr = b"LBMDEMC5", 1, 1, 1, nnbr
    H.cfg = pkg.derive(lx, ly, r)
    H.nbsteps, H.plane = 60, lx * ((ly + 15) // 16 * 16)
    rng = np.random.default_rng(n)
    lengths = [8 * n, 72 * n, 24 * n, 8 * n, 4 * (n + 1), 4 * nnbr, n, 4 * H.plane, 72 * H.plane]
    parts = [bytes(H)] + [rng.integers(0, 256, nb, dtype=np.uint8).tobytes() for nb in lengths]
    body = b"".join(parts)
    if not with_trailer:
        return body, parts
    import struct
    trailer = b"LBMCKSM1" + struct.pack("<ii", len(parts), 0)
    for p in parts:
        trailer += struct.pack("<QQQ", len(p), *digest_numpy(p))
    return body + trailer, parts


def test_verify_on_a_file_made_without_a_gpu(pkg, tmp_path):
    """n = 7 and three pairs: wallflags, offsets and nbr all end inside a 16-byte chunk, wallflags inside a word"""
    names = ("header", "r", "kin", "fhf", "gp", "offsets", "nbr", "wallflags", "obst", "f")
    data, parts = synthetic_checkpoint(pkg)
    p = tmp_path / "made.ckpt"
    p.write_bytes(data)
    assert pkg.LbmDem.checkpoint_verify(str(p)) is True
    at = 0
    for name, part in zip(names, parts):
        for where in (at, at + len(part) - 1):          # the first and the last byte of every section
            bad = bytearray(data)
            bad[where] ^= 0x10
            p.write_bytes(bytes(bad))
            with pytest.raises(pkg.LbmDemError) as e:
                pkg.LbmDem.checkpoint_verify(str(p))
            assert e.value.code == -1 and f"section '{name}'" in str(e.value), (name, where, str(e.value))
        at += len(part)
    body = data[:at]
    for keep in (len(data) - 1, at + 40, at + 8, at + 5):   # cut inside the trailer
        p.write_bytes(data[:keep])
        with pytest.raises(pkg.LbmDemError) as e:
            pkg.LbmDem.checkpoint_verify(str(p))
        assert "trailer" in str(e.value), str(e.value)
    p.write_bytes(data + b"\0")                              # something behind the trailer: not this format
    with pytest.raises(pkg.LbmDemError):
        pkg.LbmDem.checkpoint_verify(str(p))
    p.write_bytes(body)                                      # the trailer dropped whole: lbmdem_checkpoint_save's file
    assert pkg.LbmDem.checkpoint_verify(str(p)) is False
    p.write_bytes(body[:-9])                                 # ... and cut short
    with pytest.raises(pkg.LbmDemError) as e:
        pkg.LbmDem.checkpoint_verify(str(p))
    assert "shorter" in str(e.value)
    p.write_bytes(body + b"LBMDIST1" + b"\0" * 24)           # a strip's section follows: no digests, not an error
    assert pkg.LbmDem.checkpoint_verify(str(p)) is False
    assert synthetic_checkpoint(pkg, with_trailer=False)[0] == body
