"""GPU: tools/ac3mi_dec (a52dec-like file decoder on libac3mi.so) against the reference's own
liba52 + libao file drivers (oracle/_ref/a52dec_ref, built by oracle/Makefile from the reference sources), or, where
that was not built, against their output stored in tests/golden/a52dec_drivers.npz (generator: make_golden.py).  WAV
headers must be identical byte for byte; s16 samples may differ by one step (the float PCM may differ by one float32
ulp at bias 384); float output within 1e-6 RMS."""
import os
import subprocess

import numpy as np
import pytest

from tests import _harness as H

pytestmark = pytest.mark.gpu

REF_TOOL = os.path.join(H.ORACLE_DIR, "_ref", "a52dec_ref")
DRIVERS = os.path.join(H.GOLDEN, "a52dec_drivers.npz")
WAV_CASES = [("wav", "51"), ("wavdolby", "51"), ("wav6", "51"), ("wav6", "20"), ("wav6", "30"), ("wav", "20")]
FLOAT_CASES = [([], {}), (["-r"], {"no_dynrng": 1}), (["-a"], {"no_adjust": 1}), (["-g", "-6"], {"gain_db": -6.0})]


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-s", "-C", os.path.join(H.ROOT, "tools")])
    return os.path.join(H.ROOT, "tools", "ac3mi_dec")


def make_streams():
    """the test streams' bytes: 5.1, 2/0 and 3/0"""
    out = {}
    fr = H.orc_encode(H.gen_pcm(4, 6, seed=3, kind="tones"))
    out["51"] = b"\x12\x34\x0b\x76" * 5 + fr.tobytes()          # junk first: resync
    fr = H.orc_encode(H.gen_pcm(3, 2, seed=4, kind="music"), nch=2, bitrate=192000, chmap=(0, 1))
    out["20"] = fr.tobytes()
    fr = H.orc_encode(H.gen_pcm(3, 3, seed=5, kind="tones"), nch=3, bitrate=256000, chmap=(0, 2, 1))
    out["30"] = fr.tobytes()
    return out


@pytest.fixture(scope="module")
def streams(tmp_path_factory):
    d = tmp_path_factory.mktemp("tools")
    out = {}
    for key, data in make_streams().items():
        (d / (key + ".ac3")).write_bytes(data)
        out[key] = str(d / (key + ".ac3"))
    return out


def _run(tool, args, path):
    r = subprocess.run([tool] + args + [path], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert b"error" not in r.stderr
    return r.stdout


def ref_driver_name(mode, key, no_dynrng=0, no_adjust=0, gain_db=0.0):
    return "%s_%s_r%d_a%d_g%g" % (mode, key, no_dynrng, no_adjust, gain_db)


def run_ref_tool(mode, path, no_dynrng=0, no_adjust=0, gain_db=0.0):
    r = subprocess.run([REF_TOOL, mode, str(no_dynrng), str(no_adjust), str(gain_db), path], capture_output=True)
    assert r.returncode == 0 and b"errors 0" in r.stderr, r.stderr.decode()
    return r.stdout


def _ref(mode, path, **opts):
    """The reference drivers' output for one of make_streams()' streams: computed where oracle/_ref/a52dec_ref was built
    (and then equal to the stored one), else the one stored in tests/golden/a52dec_drivers.npz."""
    key = os.path.basename(path)[:-len(".ac3")]
    d = np.load(DRIVERS, allow_pickle=False)
    with open(path, "rb") as f:
        assert f.read() == d["stream_" + key].tobytes(), "stream %s differs from the one the fixture was made from" % key
    want = d[ref_driver_name(mode, key, **opts)].tobytes()
    if os.path.exists(REF_TOOL):
        assert run_ref_tool(mode, path, **opts) == want, "oracle/_ref/a52dec_ref differs from %s" % os.path.basename(DRIVERS)
    return want


@pytest.mark.parametrize("mode,key", WAV_CASES)
def test_wav_output_matches_reference_drivers(tool, streams, mode, key):
    got = _run(tool, ["-o", mode], streams[key])
    want = _ref(mode, streams[key])
    hdr = 44 if got[20:22] == b"\x01\x00" else 68
    assert got[:hdr] == want[:hdr]                       # piped: placeholder sizes, same in both
    assert len(got) == len(want) and len(got) > hdr + 6 * 256 * 2
    g = np.frombuffer(got[hdr:], "<i2").astype(np.int32)
    w = np.frombuffer(want[hdr:], "<i2").astype(np.int32)
    assert int(np.abs(g - w).max()) <= 1


def test_wav_sizes_patched_when_seekable(tool, streams, tmp_path):
    out = tmp_path / "o.wav"
    with open(out, "wb") as f:
        r = subprocess.run([tool, "-o", "wav6", streams["51"]], stdout=f, stderr=subprocess.PIPE)
    assert r.returncode == 0
    b = out.read_bytes()
    data = len(b) - 68
    assert int.from_bytes(b[4:8], "little") == data + 60 and int.from_bytes(b[64:68], "little") == data
    assert data == 4 * 6 * 256 * 6 * 2
    assert b[20:22] == b"\xfe\xff" and int.from_bytes(b[40:44], "little") == 0x3F


@pytest.mark.parametrize("args,ref_args", FLOAT_CASES)
def test_float_output_and_options(tool, streams, args, ref_args):
    got = np.frombuffer(_run(tool, ["-o", "float"] + args, streams["51"]), np.float32)
    want = np.frombuffer(_ref("float", streams["51"], **ref_args), np.float32)
    assert got.size == want.size == 4 * 6 * 512
    assert H.rms(got.astype(np.float64) - want) <= 1e-6 * max(1.0, H.rms(want) * 10)


def test_null_output_and_bad_usage(tool, streams):
    assert _run(tool, ["-o", "null6"], streams["51"]) == b""
    r = subprocess.run([tool, "-o", "nosuch", streams["51"]], capture_output=True)
    assert r.returncode == 1 and b"usage:" in r.stderr
    r = subprocess.run([tool, "-g", "200", streams["51"]], capture_output=True)
    assert r.returncode == 1 and b"Invalid gain" in r.stderr


# ---- demultiplexers (a52dec -s / -T / -t, a52dec.c:312-592): PARITY UNPINNED (src/a52dec.c cannot be built
# here); pinned property: the elementary stream recovered from a synthetic multiplex decodes to the same bytes ----

def _pes(stream_id, payload, mpeg2=True, stuffing=0, with_pts=True):
    if mpeg2:
        opt = bytes([0x21, 0x00, 0x01, 0x00, 0x01]) if with_pts else b""
        hdr = bytes([0x81, 0x80 if with_pts else 0x00, len(opt) + stuffing]) + opt + b"\xff" * stuffing
    else:                                   # MPEG-1: stuffing, optional STD buffer, PTS or the 0x0f "nothing" byte
        hdr = b"\xff" * stuffing + (bytes([0x40, 0x20]) if stuffing % 2 else b"") + \
              (bytes([0x21, 0x00, 0x01, 0x00, 0x01]) if with_pts else b"\x0f")
    body = hdr + payload
    return bytes([0, 0, 1, stream_id, len(body) >> 8, len(body) & 255]) + body


def _program_stream(es, track, rng, mpeg2=True):
    out = bytearray()
    pack = bytes([0, 0, 1, 0xBA, 0x44, 0, 4, 0, 4, 1, 1, 0x89, 0xC3, 0xF8 | 2, 0xFF, 0xFF]) if mpeg2 else \
           bytes([0, 0, 1, 0xBA, 0x21, 0, 1, 0, 1, 0x80, 0x27, 0x11])
    pos, k = 0, 0
    while pos < len(es):
        n = int(rng.integers(300, 2500))
        out += pack
        if k % 3 == 0:
            out += bytes([0, 0, 1, 0xBB, 0, 6, 0x80, 0xC4, 0xE1, 0x04, 0xE1, 0x7F])                 # system header
        out += _pes(0xE0, bytes(rng.integers(1, 255, 700, dtype=np.uint8)), mpeg2)                 # video
        other = bytes([0x80 + ((track - 0x80 + 1) % 8), 1, 0, 1]) + bytes(rng.integers(0, 256, 300, dtype=np.uint8))
        out += _pes(0xBD, other, mpeg2)                                                            # another AC-3 track
        out += _pes(0xBD, bytes([track, 1, 0, 1]) + es[pos:pos + n], mpeg2, stuffing=k % 4, with_pts=k % 2 == 0)
        out += _pes(0xBE, b"\xff" * 50, mpeg2, with_pts=False) if mpeg2 else b""                   # padding stream
        pos += n
        k += 1
    return bytes(out) + bytes([0, 0, 1, 0xB9]) + b"trailing bytes after the end code"


def _transport_stream(es, pid, rng):
    out = bytearray()
    cc = 0
    pos = 0
    while pos < len(es):
        n = int(rng.integers(500, 3000))
        pes = _pes(0xBD, es[pos:pos + n])
        pos += n
        first = True
        while pes:
            room = 184
            stuff = 0
            if len(pes) < room:
                stuff = room - len(pes)
            hdr = bytes([0x47, (0x40 if first else 0) | (pid >> 8), pid & 255, (0x30 if stuff else 0x10) | cc])
            cc = (cc + 1) & 15
            if stuff:
                af = bytes([stuff - 1]) + (bytes([0]) + b"\xff" * (stuff - 2) if stuff > 1 else b"")
                out += hdr + af + pes
                pes = b""
            else:
                out += hdr + pes[:room]
                pes = pes[room:]
            first = False
            if rng.random() < 0.3:                          # somebody else's packet
                out += bytes([0x47, 0x01, 0x00, 0x10]) + bytes(rng.integers(0, 256, 184, dtype=np.uint8))
    return bytes(out)


@pytest.mark.parametrize("kind", ["ps2", "ps1", "pes", "ts"])
def test_demultiplexers_recover_the_elementary_stream(tool, streams, tmp_path, kind):
    rng = np.random.default_rng(17)
    es = open(streams["51"], "rb").read()[20:]               # without the junk prefix
    want = _run(tool, ["-o", "wav6"], streams["51"])
    if kind == "ps2":
        data, args = _program_stream(es, 0x83, rng, True), ["-s3"]            # optional argument: attached, as in a52dec
    elif kind == "ps1":
        data, args = _program_stream(es, 0x80, rng, False), ["-s"]
    elif kind == "pes":
        data, args = b"".join(_pes(0xBD, es[i:i + 1900]) for i in range(0, len(es), 1900)), ["-T"]
    else:
        data, args = _transport_stream(es, 0x44, rng), ["-t", "0x44"]
        data = data[:188 * 3] + b"\x00" + data[188 * 3:]     # one stray byte: "bad sync byte", resynchronises
    p = tmp_path / ("in." + kind)
    p.write_bytes(data)
    r = subprocess.run([tool, "-o", "wav6"] + args + [str(p)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout[:68] == want[:68]
    if kind == "ts":
        assert b"bad sync byte" in r.stderr
        # the stray byte costs the rest of that packet's payload: at most a few frames differ in count
        assert abs(len(r.stdout) - len(want)) <= 3 * 6 * 256 * 12
    else:
        assert r.stdout == want


def test_demux_argument_checks(tool, streams):
    for bad in (["-s9"], ["-t", "5"], ["-t", "0x2000"]):
        r = subprocess.run([tool] + bad + [streams["51"]], capture_output=True)
        assert r.returncode == 1 and b"Invalid" in r.stderr
