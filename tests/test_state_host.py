"""The state blob's host side, no GPU: mmadmm_state_checksum against a Python
restatement, and mmadmm_state_info on headers written here by hand from the documented format."""
import struct

import numpy as np
import pytest

import mmadmm_amd as mx

H = mx.STATE_HEADER_BYTES
MASK = (1 << 64) - 1
# little endian: magic, version, header bytes, dim, nranks, rank, flags, nP, nF, steps taken, grid rows,
# sliding nodes, fingerprint, payload bytes, checksum, section count, reserved; then 16 x (tag[8],
# offset, bytes); 24 bytes of zeros
FIXED = "<8sIIiiiIqqqqqQQQII"
SECTION = "<8sQQ"


def checksum_py(payload):
    w = np.frombuffer(bytes(payload), dtype="<u8")
    return sum(int(x) * (2 * i + 1) for i, x in enumerate(w)) & MASK


def header(payload, sections, magic=b"MMXSTATE", version=1, hbytes=H, dim=2, nranks=1, rank=0, flags=0b001011, nP=5,
           nF=4, steps=3, rows=9, sliding=0, fp=0x0123456789ABCDEF, payload_bytes=None, checksum=None, count=None):
    out = struct.pack(FIXED, magic, version, hbytes, dim, nranks, rank, flags, nP, nF, steps, rows, sliding, fp,
                      len(payload) if payload_bytes is None else payload_bytes,
                      checksum_py(payload) if checksum is None else checksum, len(sections) if count is None else count, 0)
    for tag, off, n in sections:
        out += struct.pack(SECTION, tag, off, n)
    out += b"\0" * (H - len(out))
    assert len(out) == H
    return out


def blob_of(payload, sections, **kw):
    return np.frombuffer(header(payload, sections, **kw) + bytes(payload), dtype=np.uint8)


@pytest.fixture(scope="module")
def payload():
    return np.random.default_rng(20240611).integers(0, 256, 8 * 37, dtype=np.uint8).tobytes()


SECTIONS = [(b"x", 0, 80), (b"hess", 80, 8 * 20), (b"slAnchor", 240, 56)]


def test_checksum_equals_the_restatement(payload):
    rng = np.random.default_rng(7)
    for n in (8, 16, 8 * 1000, 8 * 4097):
        b = rng.integers(0, 256, n, dtype=np.uint8)
        assert mx.state_checksum(b) == checksum_py(b)
        assert mx.state_checksum(b.tobytes()) == checksum_py(b)
    assert mx.state_checksum(payload) == checksum_py(payload)
    assert mx.state_checksum(b"") == 0
    # all ones in every word: the weights alone, 1 + 3 + ... + (2 n - 1) = n^2 times the word, mod 2^64
    assert mx.state_checksum(b"\xff" * 80) == (MASK * 100) & MASK


def test_checksum_is_position_sensitive():
    w = np.arange(1, 65, dtype="<u8")
    p = np.random.default_rng(3).permutation(w)
    assert not np.array_equal(w, p)
    assert mx.state_checksum(w) != mx.state_checksum(p)
    assert mx.state_checksum(p) == checksum_py(p.tobytes())
    assert sum(int(x) for x in w) == sum(int(x) for x in p)  # (a plain sum would not tell them apart)


def test_checksum_refuses_a_ragged_length():
    with pytest.raises(ValueError):
        mx.state_checksum(b"1234567")
    a = np.zeros(16, dtype=np.uint8)
    assert mx.lib().mmadmm_state_checksum(a.ctypes.data, 9) == 0
    assert b"multiple of 8" in mx.lib().mmadmm_last_error()


def test_info_of_a_header_written_by_hand(payload):
    blob = blob_of(payload, SECTIONS)
    for arg in (blob, blob.tobytes(), blob[:H]):  # the whole blob (checksum verified) or the header alone
        d = mx.state_info(arg)
        assert (d["version"], d["dim"], d["nranks"], d["rank"]) == (1, 2, 1, 0)
        assert (d["nP"], d["nF"], d["steps_taken"], d["grid_rows"], d["n_sliding"]) == (5, 4, 3, 9, 0)
        assert (d["hess_computed"], d["step_taken"], d["be_step_taken"], d["regrid_each_step"], d["slide_on"],
                d["slide_frozen"]) == (True, True, False, True, False, False)
        assert d["fingerprint"] == 0x0123456789ABCDEF and d["payload_bytes"] == len(payload)
        assert d["checksum"] == checksum_py(payload) and d["n_sections"] == 3
        assert d["sections"] == {"x": (0, 80), "hess": (80, 160), "slAnchor": (240, 56)}


def test_info_from_a_file_reads_the_header_alone(payload, tmp_path):
    p = tmp_path / "hand.mmx"
    p.write_bytes(blob_of(payload, SECTIONS).tobytes())
    assert mx.state_info(p) == mx.state_info(blob_of(payload, SECTIONS))
    assert mx.state_info(str(p))["steps_taken"] == 3


def test_an_empty_payload_is_a_blob():
    d = mx.state_info(blob_of(b"", []))
    assert d["payload_bytes"] == 0 and d["checksum"] == 0 and d["sections"] == {}


CORRUPT = [
    ("magic", dict(magic=b"MMXSTATX"), "bad magic"),
    ("version", dict(version=2), "version 2 is newer"),
    ("version0", dict(version=0), "version"),
    ("header size", dict(hbytes=256), "header size"),
    ("count", dict(count=17), "section count"),
    ("checksum", dict(checksum=1), "wrong checksum"),
    ("payload bytes", dict(payload_bytes=8 * 36), "does not tile"),
]


@pytest.mark.parametrize("what,kw,msg", CORRUPT, ids=[c[0] for c in CORRUPT])
def test_corrupted_headers_are_refused(payload, what, kw, msg):
    with pytest.raises(mx.MMADMMError, match=msg) as e:
        mx.state_info(blob_of(payload, SECTIONS, **kw))
    assert e.value.code == 1


def test_section_tables_that_do_not_tile_are_refused(payload):
    gap = [(b"x", 0, 80), (b"hess", 88, 152), (b"slAnchor", 240, 56)]
    overlap = [(b"x", 0, 88), (b"hess", 80, 160), (b"slAnchor", 240, 56)]
    short = SECTIONS[:2]
    ragged = [(b"x", 0, 84), (b"hess", 84, 156), (b"slAnchor", 240, 56)]
    for sections in (gap, overlap, short, ragged):
        with pytest.raises(mx.MMADMMError, match="does not tile the payload"):
            mx.state_info(blob_of(payload, sections))


def test_lengths_are_checked(payload):
    blob = blob_of(payload, SECTIONS)
    with pytest.raises(mx.MMADMMError, match="too short"):
        mx.state_info(blob[:-8])
    with pytest.raises(mx.MMADMMError, match="too long"):
        mx.state_info(np.concatenate([blob, np.zeros(8, np.uint8)]))
    with pytest.raises(mx.MMADMMError, match="shorter than the 512-byte header"):
        mx.state_info(blob[:H - 1])
    L = mx.lib()
    hdr = mx.mmadmm_state_header()
    assert L.mmadmm_state_info(None, H, hdr) == 1 and b"NULL" in L.mmadmm_last_error()
    assert L.mmadmm_state_info(blob.ctypes.data, blob.size, None) == 1 and b"NULL" in L.mmadmm_last_error()
