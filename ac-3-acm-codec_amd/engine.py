"""Host-side mirror of the batched engine: torch tensors in, torch tensors out.

torch is plumbing here (device memory + dtype checks); every computation happens
in libac3mi.so.  Mirrors the stage boundaries of the reference:
``Engine.imdct_batch`` = the synthesis stage of a52_block (liba52/parse.c:881-937).
"""
import ctypes
from dataclasses import dataclass

from . import capi


@dataclass
class XformDesc:
    acmod: int = 7
    lfeon: int = 1
    output: int = 7 | 16
    bias: float = 0.0

    def c(self):
        return capi.XformDescC(self.acmod, self.lfeon, self.output, self.bias)


@dataclass
class DecodeDesc:
    """Arguments of a52_frame() plus the coded configuration a52_syncinfo() reported."""
    flags: int = 7 | 16
    level: float = 1.0
    bias: float = 0.0
    dynrng: int = 1
    acmod: int = 7
    lfeon: int = 1
    frame_bytes: int = 1536

    def c(self):
        return capi.DecodeDescC(self.flags, self.level, self.bias, self.dynrng, self.acmod, self.lfeon,
                                self.frame_bytes)


@dataclass
class EncodeDesc:
    """AC3_encode_init's arguments (src/ac3enc/ac3enc.h:6)."""
    sample_rate: int = 48000
    bit_rate: int = 384000
    channels: int = 6

    def c(self):
        return capi.EncodeDescC(self.sample_rate, self.bit_rate, self.channels)

    def frame_bytes(self):
        c = self.c()
        return capi.load_library().ac3mi_encode_frame_bytes(ctypes.byref(c))


def syncinfo(buf):
    """a52_syncinfo on host bytes -> (frame_bytes, flags, sample_rate, bit_rate); frame_bytes 0 = no frame."""
    lib = capi.load_library()
    b = (ctypes.c_uint8 * 8)(*bytes(buf[:8]))
    fl, sr, br = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    n = lib.ac3mi_syncinfo(b, ctypes.byref(fl), ctypes.byref(sr), ctypes.byref(br))
    return n, fl.value, sr.value, br.value


def bsi_read(buf):
    """ac3mi_bsi_read on host bytes (a frame, or only its head) -> a numpy record of capi.bsi_info_dtype()."""
    import numpy as np
    lib = capi.load_library()
    data = bytes(bytearray(buf))
    b = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    info = capi.BsiInfoC()
    if lib.ac3mi_bsi_read(b, len(data), ctypes.byref(info)) != 0:
        raise capi.AC3MIError("ac3mi_bsi_read: bad argument")
    return np.frombuffer(bytes(info), capi.bsi_info_dtype())[0]


def frame_scan(buf, mode=0, max_frames=None):
    """ac3mi_frame_scan on host bytes: the frames of a byte stream by the reference's resync rule (mode 1: a candidate counts
    only if both of its CRC regions check) -> (refs, info): numpy records of capi.frame_ref_dtype() [n_frames] and one of
    capi.scan_info_dtype().  max_frames: room in the list, default every frame the bytes can hold."""
    import numpy as np
    lib = capi.load_library()
    data = bytes(bytearray(buf))
    if max_frames is None:
        max_frames = len(data) // 128 + 1
    b = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    refs = (capi.FrameRefC * max(1, int(max_frames)))()
    info = capi.ScanInfoC()
    if lib.ac3mi_frame_scan(b, len(data), int(mode), int(max_frames), refs, ctypes.byref(info)) != 0:
        raise capi.AC3MIError("ac3mi_frame_scan: bad argument")
    out = np.frombuffer(bytes(info), capi.scan_info_dtype())[0]
    return np.frombuffer(bytes(refs), capi.frame_ref_dtype())[:int(out["n_frames"])].copy(), out


def _read_host(entry_name, state_bytes_name, ResultC, dtype, state, *extra, what="state"):
    """A PCM tool's host read-out: one state's bytes, then `extra`, -> a numpy record of dtype"""
    import numpy as np
    lib = capi.load_library()
    data = bytes(bytearray(state))
    nb = getattr(lib, state_bytes_name)()
    if len(data) != nb:
        raise ValueError("a %s is %d bytes" % (what, nb))
    res = ResultC()
    if getattr(lib, entry_name)(data, *extra, ctypes.byref(res)) != 0:
        raise capi.AC3MIError(entry_name + ": bad argument")
    return np.frombuffer(bytes(res), dtype)[0]


def _roles_array(roles, nch):
    """one role per channel -> the uint8 [6] the C entries take"""
    if len(roles) != nch:
        raise ValueError("one role per channel")
    return (ctypes.c_uint8 * 6)(*(list(roles) + [0] * 6)[:6])


def _host_stream(pcm, state, state_bytes, roles=None):
    """A PCM tool's host twin works on ONE stream: pcm -> int16 [frames * 1536][channels], contiguous; the state's bytes (None:
    a new stream) -> a buffer of state_bytes that the call updates"""
    import numpy as np
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    if pcm.ndim != 2 or pcm.shape[0] % 1536 or (roles is not None and len(roles) != pcm.shape[1]):
        raise ValueError("pcm is [frames * 1536][channels]" + (", one role per channel" if roles is not None else ""))
    return pcm, ctypes.create_string_buffer(bytes(bytearray(state)) if state is not None else bytes(state_bytes), state_bytes)


def loudness_state_bytes():
    """ac3mi_loudness_state_bytes: bytes of one stream's meter state (all zeros: a new stream)"""
    return int(capi.load_library().ac3mi_loudness_state_bytes())


def loudness_roles(a52_flags):
    """ac3mi_loudness_roles: the roles (0 not measured, 1 weight 1.0, 2 weight 1.41) of the WAVE-order slots that the s16
    decoders write for these liba52 output flags -> a list, one per channel"""
    role = (ctypes.c_uint8 * 6)()
    n = capi.load_library().ac3mi_loudness_roles(int(a52_flags), role)
    if n <= 0:
        raise capi.AC3MIError("ac3mi_loudness_roles: no layout for flags %d" % a52_flags)
    return list(role)[:n]


def loudness_tables(sample_rate):
    """ac3mi_loudness_tables -> (coef float64 [10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2; bin edges [901];
    dialnorm thresholds [30])"""
    import numpy as np
    coef, edges, thr = np.zeros(10), np.zeros(901), np.zeros(30)
    if capi.load_library().ac3mi_loudness_tables(int(sample_rate), coef.ctypes.data, edges.ctypes.data, thr.ctypes.data) != 0:
        raise capi.AC3MIError("ac3mi_loudness_tables: %r is not a rate the meter takes" % (sample_rate,))
    return coef, edges, thr


def loudness_read(state):
    """ac3mi_loudness_read, the host read-out: one state's bytes (ac3mi_loudness_state_bytes of them) -> a numpy record of
    capi.loudness_result_dtype()"""
    return _read_host("ac3mi_loudness_read", "ac3mi_loudness_state_bytes", capi.LoudnessResultC, capi.loudness_result_dtype(), state)


def loudness_range_state_bytes():
    """ac3mi_loudness_range_state_bytes: bytes of one stream's range-meter state (all zeros: a new stream)"""
    return int(capi.load_library().ac3mi_loudness_range_state_bytes())


def loudness_range_read(state):
    """ac3mi_loudness_range_read, the host read-out: one range state's bytes (ac3mi_loudness_range_state_bytes of them) -> a
    numpy record of capi.loudness_range_result_dtype()"""
    return _read_host("ac3mi_loudness_range_read", "ac3mi_loudness_range_state_bytes", capi.LoudnessRangeResultC,
                      capi.loudness_range_result_dtype(), state, what="range state")


def truepeak_state_bytes():
    """ac3mi_truepeak_state_bytes: bytes of one stream's true-peak state (all zeros: a new stream)"""
    return int(capi.load_library().ac3mi_truepeak_state_bytes())


def truepeak_tables():
    """ac3mi_truepeak_tables -> H int16 [4][12]: BS.1770-4 Annex 2's interpolator by phase, times 8192"""
    import numpy as np
    h = np.zeros((4, 12), np.int16)
    if capi.load_library().ac3mi_truepeak_tables(h.ctypes.data) != 0:
        raise capi.AC3MIError("ac3mi_truepeak_tables: bad argument")
    return h


def truepeak_ceiling(dbtp):
    """ac3mi_truepeak_ceiling: a ceiling in dBTP -> the integer (2^-28 of full scale) that the read-out compares with"""
    return int(capi.load_library().ac3mi_truepeak_ceiling(float(dbtp)))


def truepeak_read(state, ceiling_q28=0):
    """ac3mi_truepeak_read, the host read-out: one state's bytes (ac3mi_truepeak_state_bytes of them) -> a numpy record of
    capi.truepeak_result_dtype()"""
    return _read_host("ac3mi_truepeak_read", "ac3mi_truepeak_state_bytes", capi.TruePeakResultC, capi.truepeak_result_dtype(), state,
                      int(ceiling_q28))


def truepeak_host(roles, pcm, state=None):
    """ac3mi_truepeak_host, the host meter (no GPU): pcm int16 [n][channels] of ONE stream, n a multiple of 1536, on the
    state's bytes (None: a new stream) -> the new state's bytes.  roles: 0 = not measured, else measured, one per channel."""
    lib = capi.load_library()
    pcm, buf = _host_stream(pcm, state, lib.ac3mi_truepeak_state_bytes(), roles)
    if lib.ac3mi_truepeak_host(int(pcm.shape[1]), _roles_array(roles, pcm.shape[1]), pcm.ctypes.data, pcm.shape[0] // 1536, buf) != 0:
        raise capi.AC3MIError("ac3mi_truepeak_host: bad argument")
    return buf.raw


def limit_state_bytes():
    """ac3mi_limit_state_bytes: bytes of one stream's limiter state (all zeros: a new stream)"""
    return int(capi.load_library().ac3mi_limit_state_bytes())


def limit_release_step(sample_rate, full_recovery_ms):
    """ac3mi_limit_release_step: the Q24 gain step per sample that recovers full scale in full_recovery_ms, in [1, 2^20]"""
    return int(capi.load_library().ac3mi_limit_release_step(int(sample_rate), float(full_recovery_ms)))


def limit_read(state):
    """ac3mi_limit_read, the host read-out: one state's bytes (ac3mi_limit_state_bytes of them) -> a numpy record of
    capi.limit_result_dtype()"""
    return _read_host("ac3mi_limit_read", "ac3mi_limit_state_bytes", capi.LimitResultC, capi.limit_result_dtype(), state)


def limit_host(roles, ceiling_q28, release_step_q24, pcm, state=None):
    """ac3mi_limit_host, the host limiter (no GPU): pcm int16 [n][channels] of ONE stream, n a multiple of 1536, on the
    state's bytes (None: a new stream) -> (out int16 [n][channels], the new state's bytes).  roles: 0 = not detected, else
    detected, one per channel; every channel is delayed by 77 samples and gets the gain."""
    import numpy as np
    lib = capi.load_library()
    pcm, buf = _host_stream(pcm, state, lib.ac3mi_limit_state_bytes(), roles)
    out = np.empty_like(pcm)
    if lib.ac3mi_limit_host(int(pcm.shape[1]), _roles_array(roles, pcm.shape[1]), int(ceiling_q28), int(release_step_q24), pcm.ctypes.data,
                            out.ctypes.data, pcm.shape[0] // 1536, buf) != 0:
        raise capi.AC3MIError("ac3mi_limit_host: bad argument")
    return out, buf.raw


ResampleDesc = capi.ResampleDescC


def resample_ratio(in_rate, out_rate):
    """ac3mi_resample_ratio: (L, M, taps per phase) of one of the six pairs of {32000, 44100, 48000}"""
    L, M, T = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if capi.load_library().ac3mi_resample_ratio(int(in_rate), int(out_rate), ctypes.byref(L), ctypes.byref(M), ctypes.byref(T)) != 0:
        raise capi.AC3MIError("ac3mi_resample_ratio: bad argument")
    return L.value, M.value, T.value


def resample_tables(in_rate, out_rate):
    """ac3mi_resample_tables: the pair's Q23 table, int32 [L][taps]"""
    import numpy as np
    L, _, T = resample_ratio(in_rate, out_rate)
    coef = np.zeros((L, T), np.int32)
    rc = capi.load_library().ac3mi_resample_tables(int(in_rate), int(out_rate), coef.ctypes.data)
    if rc != 0:
        raise capi.AC3MIError("ac3mi_resample_tables: %d" % rc)
    return coef


def resample_state_bytes():
    """ac3mi_resample_state_bytes: bytes of one stream's converter state (all zeros: a new stream)"""
    return int(capi.load_library().ac3mi_resample_state_bytes())


def resample_plan(in_rate, out_rate, samples_in, frames_out, in_frames):
    """ac3mi_resample_plan: (out_frames, pending_after) of a call that pushes in_frames frames to a stream of that age"""
    of, left = ctypes.c_int(), ctypes.c_int()
    if capi.load_library().ac3mi_resample_plan(int(in_rate), int(out_rate), int(samples_in), int(frames_out), int(in_frames),
                                               ctypes.byref(of), ctypes.byref(left)) != 0:
        raise capi.AC3MIError("ac3mi_resample_plan: bad argument")
    return of.value, left.value


def resample_host(desc, pcm, out_frames, state=None):
    """ac3mi_resample_host, the host converter (no GPU): pcm int16 [n][channels] of ONE stream, n a multiple of 1536, on the
    state's bytes (None: a new stream) -> (out int16 [out_frames * 1536][channels], the state's bytes, status).  desc: a
    ResampleDesc or (in_rate, out_rate)."""
    import numpy as np
    lib = capi.load_library()
    pcm, buf = _host_stream(pcm, state, lib.ac3mi_resample_state_bytes())
    if not isinstance(desc, capi.ResampleDescC):
        desc = capi.ResampleDescC(int(desc[0]), int(desc[1]), int(pcm.shape[1]))
    out = np.full((int(out_frames) * 1536, pcm.shape[1]), 0x5a5a, np.int16)
    status = ctypes.c_uint32(0xffffffff)
    if lib.ac3mi_resample_host(ctypes.byref(desc), pcm.ctypes.data, pcm.shape[0] // 1536, out.ctypes.data if out.size else None,
                               int(out_frames), buf, ctypes.byref(status)) != 0:
        raise capi.AC3MIError("ac3mi_resample_host: bad argument")
    return out, buf.raw, int(status.value)


def encode_metadata_word(**fields):
    """ac3mi_encode_metadata_word: the fields of Engine.set_encode_metadata (those not given: the defaults) -> the packed
    word; raises on a field out of range."""
    unknown = set(fields) - set(Engine._METADATA_FIELDS)
    if unknown:
        raise TypeError("unknown metadata field(s): %s" % ", ".join(sorted(unknown)))
    md = (ctypes.c_int * 7)(*[int(fields.get(k, d)) for k, d in zip(Engine._METADATA_FIELDS, Engine._METADATA_DEFAULTS)])
    w = ctypes.c_uint32()
    if capi.load_library().ac3mi_encode_metadata_word(ctypes.cast(md, ctypes.c_void_p), ctypes.byref(w)) != 0:
        raise capi.AC3MIError("ac3mi_encode_metadata_word: field out of range")
    return w.value


class Engine:
    def __init__(self, device=0):
        self.lib = capi.load_library()
        self.ctx = self.lib.ac3mi_create(device)
        if not self.ctx:
            raise capi.AC3MIError(self.lib.ac3mi_last_error(None).decode())
        self.device = device
        # tensors handed to in-flight launches: torch's caching allocator only orders reuse on
        # torch's own stream, so keep them alive until the engine stream has been drained
        self._keep = []

    def close(self):
        if self.ctx:
            self.lib.ac3mi_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise capi.AC3MIError("ac3mi error %d: %s" % (rc, self.lib.ac3mi_last_error(self.ctx).decode()))

    def _drain_torch(self, wait_torch):
        """The engine launches on its own (non-blocking) HIP streams.  Everything torch has queued for the buffers of a
        call - the producers of its inputs AND the fills of outputs allocated inside the call (torch.zeros) - must have
        finished before the engine touches them, so the drain comes after every allocation, right before the launch."""
        if wait_torch:
            import torch
            torch.cuda.synchronize(self.device)

    def sync(self):
        self._check(self.lib.ac3mi_sync(self.ctx))
        self._keep.clear()

    def memset(self, t, byte=0):
        """ac3mi_memset of a whole tensor on the engine's stream (asynchronous)."""
        self._check(self.lib.ac3mi_memset(ctypes.c_void_p(self.ctx), ctypes.c_void_p(t.data_ptr()), int(byte), ctypes.c_size_t(t.numel() * t.element_size())))

    def copy(self, dst, src):
        """ac3mi_memcpy_d2d of a whole tensor on the engine's stream (asynchronous)."""
        assert dst.numel() * dst.element_size() == src.numel() * src.element_size()
        self._check(self.lib.ac3mi_memcpy_d2d(ctypes.c_void_p(self.ctx), ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()),
                                              ctypes.c_size_t(dst.numel() * dst.element_size())))

    def timer_start(self):
        self._check(self.lib.ac3mi_timer_start(self.ctx))

    def timer_stop(self):
        ms = ctypes.c_float()
        self._check(self.lib.ac3mi_timer_stop(self.ctx, ctypes.byref(ms)))
        self._keep.clear()
        return ms.value

    def planes(self, desc):
        n_in, n_out = ctypes.c_int(), ctypes.c_int()
        c = desc.c()
        rc = self.lib.ac3mi_xform_planes(ctypes.byref(c), ctypes.byref(n_in), ctypes.byref(n_out))
        if rc != 0:
            raise capi.AC3MIError("output flags %d not reachable from acmod %d" % (desc.output, desc.acmod))
        return n_in.value, n_out.value

    def imdct_batch(self, desc, coeffs, delay, blksw=None, out=None, wait_torch=True):
        """coeffs [S][F][6][n_in][256] f32, delay [S][n_out][128] f32 (updated in place),
        blksw None or [S][F][6][nfchans] u8  ->  pcm [S][F][6][n_out][256] f32.

        The engine runs on its own HIP stream: with wait_torch the call first drains torch's
        stream (the inputs were produced there); call sync() before reading the result."""
        import torch
        n_in, n_out = self.planes(desc)
        S, F = coeffs.shape[0], coeffs.shape[1]
        assert coeffs.dtype == torch.float32 and coeffs.is_contiguous() and coeffs.is_cuda
        assert tuple(coeffs.shape) == (S, F, 6, n_in, 256), coeffs.shape
        assert delay.dtype == torch.float32 and delay.is_contiguous() and tuple(delay.shape) == (S, n_out, 128)
        if blksw is not None:
            assert blksw.dtype == torch.uint8 and blksw.is_contiguous() and blksw.shape[:3] == (S, F, 6)
        if out is None:
            out = torch.empty((S, F, 6, n_out, 256), dtype=torch.float32, device=coeffs.device)
        c = desc.c()
        self._drain_torch(wait_torch)
        self._check(self.lib.ac3mi_imdct_batch(self.ctx, ctypes.byref(c), coeffs.data_ptr(),
                                               blksw.data_ptr() if blksw is not None else None,
                                               delay.data_ptr(), out.data_ptr(), S, F))
        self._keep.append((coeffs, delay, blksw, out))
        return out

    def decode_planes(self, desc):
        n_out, fl = ctypes.c_int(), ctypes.c_int()
        c = desc.c()
        if self.lib.ac3mi_decode_planes(ctypes.byref(c), ctypes.byref(n_out), ctypes.byref(fl)) != 0:
            raise capi.AC3MIError("a52_frame would refuse flags %d for acmod %d" % (desc.flags, desc.acmod))
        return n_out.value, fl.value

    def decode_batch(self, desc, frames, delay, lfsr, out=None, status=None, taps=False, wait_torch=True, dynrng_in=None):
        """frames [S][F][stride] u8 (stride multiple of 4), delay [S][n_out][128] f32, lfsr [S] i16/u16
        (both updated in place) -> (pcm [S][F][6][n_out][256] f32, status [S][F] i32[, taps dict])."""
        import torch
        n_out, out_flags = self.decode_planes(desc)
        S, F, stride = frames.shape
        assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.is_cuda
        assert delay.dtype == torch.float32 and tuple(delay.shape) == (S, n_out, 128) and delay.is_contiguous()
        assert lfsr.dtype in (torch.int16, torch.uint16) and tuple(lfsr.shape) == (S,)
        dev = frames.device
        if out is None:
            out = torch.empty((S, F, 6, n_out, 256), dtype=torch.float32, device=dev)
        if status is None:
            status = torch.zeros((S, F), dtype=torch.int32, device=dev)
        nf = (2, 1, 2, 3, 3, 4, 4, 5)[desc.acmod]
        n_in = nf + (1 if desc.lfeon else 0)
        tp, tdict = None, None
        if taps:
            tdict = {
                "coef": torch.zeros((S, F, 6, n_in, 256), dtype=torch.float32, device=dev),
                "blksw": torch.zeros((S, F, 6, nf), dtype=torch.uint8, device=dev),
                "exp": torch.zeros((S, F, 6, 7, 256), dtype=torch.uint8, device=dev),
                "bap": torch.zeros((S, F, 6, 7, 256), dtype=torch.int8, device=dev),
            }
            tdict["dynrng"] = torch.full((S, F, 6, 2), float("nan"), dtype=torch.float32, device=dev)
            tp = capi.DecodeTapsC(tdict["coef"].data_ptr(), tdict["blksw"].data_ptr(), tdict["exp"].data_ptr(),
                                  tdict["bap"].data_ptr(), tdict["dynrng"].data_ptr(),
                                  dynrng_in.data_ptr() if dynrng_in is not None else None)
        c = desc.c()
        self._drain_torch(wait_torch or taps)
        self._check(self.lib.ac3mi_decode_batch(self.ctx, ctypes.byref(c), frames.data_ptr(), stride, S, F,
                                                delay.data_ptr(), lfsr.data_ptr(), out.data_ptr(),
                                                status.data_ptr(), ctypes.byref(tp) if tp else None))
        self._keep.append((frames, delay, lfsr, out, status, tdict))
        if taps:
            return out, status, tdict
        return out, status

    def decode_s16_batch(self, desc, frames, delay, lfsr, out=None, status=None, wait_torch=True):
        """ac3mi_decode_s16_batch: like decode_batch at level 1 / bias 384 with the reference's s16 converter folded into
        the transform -> (pcm [S][F][6][256][n_out] i16 in WAVE channel order, status [S][F] i32)."""
        import torch
        n_out, _ = self.decode_planes(desc)
        S, F, stride = frames.shape
        assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.is_cuda
        assert delay.dtype == torch.float32 and tuple(delay.shape) == (S, n_out, 128) and delay.is_contiguous()
        assert lfsr.dtype in (torch.int16, torch.uint16) and tuple(lfsr.shape) == (S,)
        dev = frames.device
        if out is None:
            out = torch.empty((S, F, 6, 256, n_out), dtype=torch.int16, device=dev)
        if status is None:
            status = torch.zeros((S, F), dtype=torch.int32, device=dev)
        c = desc.c()
        self._drain_torch(wait_torch)
        self._check(self.lib.ac3mi_decode_s16_batch(self.ctx, ctypes.byref(c), frames.data_ptr(), stride, S, F,
                                                    delay.data_ptr(), lfsr.data_ptr(), out.data_ptr(), status.data_ptr()))
        self._keep.append((frames, delay, lfsr, out, status))
        return out, status

    def probe_valu_rate(self):
        """10^9 VALU instructions/s one SIMD sustains under a chip-wide VALU load (ac3mi_probe_valu_rate)."""
        v = ctypes.c_double()
        self._check(self.lib.ac3mi_probe_valu_rate(ctypes.c_void_p(self.ctx), ctypes.byref(v)))
        return v.value

    def probe_copy_rate(self, nbytes=1 << 31):
        """GB/s (read + written) of a bare one-float4-per-lane copy of nbytes (ac3mi_probe_copy_rate)."""
        v = ctypes.c_double(0.0)
        self._check(self.lib.ac3mi_probe_copy_rate(ctypes.c_void_p(self.ctx), ctypes.c_size_t(int(nbytes)), ctypes.byref(v)))
        return v.value

    def probe_salu_rate(self):
        """10^9 scalar instructions/s one SIMD's share of the scalar unit sustains under a chip-wide load (ac3mi_probe_salu_rate)."""
        v = ctypes.c_double()
        self._check(self.lib.ac3mi_probe_salu_rate(ctypes.c_void_p(self.ctx), ctypes.byref(v)))
        return v.value

    def probe_mixed_rate(self, waves_per_simd=8):
        """(vector, scalar) 10^9 instructions/s per SIMD when every wavefront issues three vector instructions per scalar one
        (ac3mi_probe_mixed_rate)."""
        v, s = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.ac3mi_probe_mixed_rate(ctypes.c_void_p(self.ctx), int(waves_per_simd), ctypes.byref(v), ctypes.byref(s)))
        return v.value, s.value

    def workspace_bytes(self):
        """Device bytes the context's workspaces hold right now (ac3mi_workspace_bytes)."""
        self.lib.ac3mi_workspace_bytes.restype = ctypes.c_size_t
        return int(self.lib.ac3mi_workspace_bytes(ctypes.c_void_p(self.ctx)))

    def fill_workspaces(self, byte):
        """Test aid: fills every workspace the context holds right now with `byte` (0..255) on the engine's stream
        (ac3mi_fill_workspaces); a call's results must not depend on it."""
        self._check(self.lib.ac3mi_fill_workspaces(ctypes.c_void_p(self.ctx), int(byte)))

    def set_tile_frames(self, frames):
        """Workspace bound: batches above `frames` frames go through in tiles of whole streams (ac3mi_set_tile_frames)."""
        self._check(self.lib.ac3mi_set_tile_frames(ctypes.c_void_p(self.ctx), int(frames)))

    def set_decode_mode(self, mode):
        """0 = choose by batch shape, 1 = one wavefront per stream (one-kernel reference), 3 = one workgroup per stream with the
        transform fused in, 4 / 5 = parse kernel per stream / per frame + one wavefront per audio block, 6 = as 4 with the transform
        in the mantissa kernel for one-frame streams without a downmix (ac3mi_set_decode_mode)."""
        self._check(self.lib.ac3mi_set_decode_mode(ctypes.c_void_p(self.ctx), int(mode)))

    def set_fixed_shape(self, on):
        """1 (default) = 5.1 calls take the kernels that have that shape compiled in where their stage allows it, 0 = always the
        generic kernels; the bytes are the same (ac3mi_set_fixed_shape)."""
        self._check(self.lib.ac3mi_set_fixed_shape(ctypes.c_void_p(self.ctx), int(on)))

    def debug_search_curve(self, curve):
        """Test aid (ac3mi_debug_search_curve): `curve` = an int32 CUDA tensor [streams][frames][1024][2] that the encoder's
        SNR-offset search of the following encode / transcode calls fills, for every offset it costs, with the frame's spare
        bits and ceiling sixths there, or None to end the tap.  The caller keeps the tensor alive while the tap is set."""
        self._check(self.lib.ac3mi_debug_search_curve(ctypes.c_void_p(self.ctx), ctypes.c_void_p(curve.data_ptr() if curve is not None else None)))

    def debug_launch_log(self, log):
        """Test aid (ac3mi_debug_launch_log): `log` = a C-contiguous uint32 numpy array in host memory that the following
        decode / encode / transcode calls fill - log[0] counts the launches of the launch rule's kernels since the tap was
        set, log[1:] holds family << 24 | variant word of each in launch order - or None to end the tap.  The caller keeps
        the array alive while the tap is set."""
        if log is None:
            self._check(self.lib.ac3mi_debug_launch_log(ctypes.c_void_p(self.ctx), None, 0))
            return
        import numpy as np
        assert isinstance(log, np.ndarray) and log.dtype == np.uint32 and log.flags.c_contiguous and log.flags.writeable and log.ndim == 1
        self._check(self.lib.ac3mi_debug_launch_log(ctypes.c_void_p(self.ctx), ctypes.c_void_p(log.ctypes.data), int(log.size)))

    def set_decode_crc(self, mode):
        """CRC verification of the frames the decode and transcode calls read (ac3mi_set_decode_crc): 0 = none (liba52),
        1 = report in status bits 10 / 11 (flags.STATUS_CRC1 / STATUS_CRC2), 2 = also decode a failing frame as a refused
        one (silence, status 0x13f plus its CRC bits)."""
        self._check(self.lib.ac3mi_set_decode_crc(ctypes.c_void_p(self.ctx), int(mode)))

    def crc_check_batch(self, frames, frame_bytes=None, out=None, wait_torch=True):
        """ac3mi_crc_check_batch: frames [...][stride] u8 on the device (stride multiple of 4; frame_bytes = the largest
        frame's size, default the stride) -> verdict u8 [...]: bit 0 CRC1 fails, bit 1 CRC2 fails, bit 7 not summed."""
        import torch
        assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.is_cuda and frames.dim() >= 2
        stride = frames.shape[-1]
        n = frames.numel() // stride if stride else 0
        if out is None:
            out = torch.zeros(tuple(frames.shape[:-1]), dtype=torch.uint8, device=frames.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n
        self._drain_torch(wait_torch)
        self._check(self.lib.ac3mi_crc_check_batch(ctypes.c_void_p(self.ctx), ctypes.c_void_p(frames.data_ptr()), int(stride),
                                                   int(stride if frame_bytes is None else frame_bytes), ctypes.c_size_t(n),
                                                   ctypes.c_void_p(out.data_ptr())))
        self._keep.append((frames, out))
        return out

    def set_encode_mode(self, mode):
        """0 = choose by batch size, 1 = one wavefront per frame packs, 2 = one wavefront per audio block packs
        (ac3mi_set_encode_mode)."""
        self._check(self.lib.ac3mi_set_encode_mode(ctypes.c_void_p(self.ctx), int(mode)))

    def set_encode_block_switch(self, mode):
        """0 = long blocks only (the reference), 1 = a transient detector switches channel-blocks to the short transform
        pair (ac3mi_set_encode_block_switch).  Applies to encode_batch and transcode_batch."""
        self._check(self.lib.ac3mi_set_encode_block_switch(ctypes.c_void_p(self.ctx), int(mode)))

    def set_encode_rematrix(self, mode):
        """0 = no rematrixing (the reference), 1 = 2/0 frames code (L+R)/2 and (L-R)/2 in the bands where that pays
        (ac3mi_set_encode_rematrix).  Applies to encode_batch and transcode_batch."""
        self._check(self.lib.ac3mi_set_encode_rematrix(ctypes.c_void_p(self.ctx), int(mode)))

    def set_encode_coupling(self, mode, begf=0):
        """0 = every channel coded on its own (the reference), 1 = frames with two or more full-bandwidth channels couple them
        above sub-band `begf` (0..12; cplstrtmant = 37 + 12 begf) where the rule of ac3mi_set_encode_coupling allows.
        Applies to encode_batch and transcode_batch."""
        self._check(self.lib.ac3mi_set_encode_coupling(ctypes.c_void_p(self.ctx), int(mode), int(begf)))

    def set_encode_bandwidth(self, mode, chbwcod=50):
        """0 = chbwcod 50, bins [0, 223) (the reference), 1 = every full-bandwidth channel codes [0, 73 + 3 chbwcod) with `chbwcod`
        (0..50), 2 = chbwcod follows each call's bit rate per full-bandwidth channel and sample rate (ac3mi_set_encode_bandwidth).
        Applies to encode_batch and transcode_batch."""
        self._check(self.lib.ac3mi_set_encode_bandwidth(ctypes.c_void_p(self.ctx), int(mode), int(chbwcod)))

    _METADATA_FIELDS = ("dialnorm", "bsmod", "cmixlev", "surmixlev", "dsurmod", "copyrightb", "origbs")
    _METADATA_DEFAULTS = (31, 0, 1, 1, 0, 0, 1)

    def set_encode_metadata(self, **fields):
        """BSI fields of the encoded frames (ac3mi_set_encode_metadata): dialnorm 1..31, bsmod 0..7, cmixlev / surmixlev /
        dsurmod 0..2, copyrightb / origbs 0/1; fields not given take their defaults (31, 0, 1, 1, 0, 0, 1), no fields
        restores the defaults.  Applies to encode_batch and transcode_batch."""
        unknown = set(fields) - set(self._METADATA_FIELDS)
        if unknown:
            raise TypeError("unknown metadata field(s): %s" % ", ".join(sorted(unknown)))
        if not fields:
            self._check(self.lib.ac3mi_set_encode_metadata(ctypes.c_void_p(self.ctx), None))
            return
        vals = [int(fields.get(k, d)) for k, d in zip(self._METADATA_FIELDS, self._METADATA_DEFAULTS)]
        md = (ctypes.c_int * 7)(*vals)
        self._check(self.lib.ac3mi_set_encode_metadata(ctypes.c_void_p(self.ctx), ctypes.cast(md, ctypes.c_void_p)))

    def set_encode_metadata_frames(self, words=None):
        """BSI metadata per frame (ac3mi_set_encode_metadata_frames): `words` int32 / uint32 [S][F] on the device, one
        encode_metadata_word per frame of the following encode_batch / transcode_batch calls (sanitised by the engine; kept
        referenced while set); None returns to the context's one word."""
        if words is not None:
            import torch
            if words.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not words.is_cuda or not words.is_contiguous():
                raise ValueError("words must be a contiguous int32 / uint32 tensor on the device")
            torch.cuda.current_stream().synchronize()       # their fill was queued on torch's stream
        self._check(self.lib.ac3mi_set_encode_metadata_frames(ctypes.c_void_p(self.ctx),
                                                              ctypes.c_void_p(words.data_ptr()) if words is not None else None))
        self._md_words = words

    def set_encode_metadata_source(self, mode):
        """Where transcode_batch takes the new frames' BSI metadata from (ac3mi_set_encode_metadata_source): 0 = the context's
        settings, 1 = each source frame's own BSI (flags.MD_SOURCE_FOLLOW)."""
        self._check(self.lib.ac3mi_set_encode_metadata_source(ctypes.c_void_p(self.ctx), int(mode)))

    def bsi_read_batch(self, frames, frame_bytes=None, out=None, wait_torch=True):
        """ac3mi_bsi_read_batch: frames [...][stride] u8 on the device (stride multiple of 4; frame_bytes = the largest frame's
        size, default the stride) -> records u8 [...][36]; `.cpu().numpy().view(capi.bsi_info_dtype())[..., 0]` names the fields."""
        import torch
        assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.is_cuda and frames.dim() >= 2
        stride = frames.shape[-1]
        n = frames.numel() // stride if stride else 0
        size = ctypes.sizeof(capi.BsiInfoC)
        if out is None:
            out = torch.zeros(tuple(frames.shape[:-1]) + (size,), dtype=torch.uint8, device=frames.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * size
        self._drain_torch(wait_torch)
        self._check(self.lib.ac3mi_bsi_read_batch(ctypes.c_void_p(self.ctx), ctypes.c_void_p(frames.data_ptr()), int(stride),
                                                  int(stride if frame_bytes is None else frame_bytes), ctypes.c_size_t(n),
                                                  ctypes.c_void_p(out.data_ptr())))
        self._keep.append((frames, out))
        return out

    def frame_scan_batch(self, streams, lens, mode=0, max_frames=16, refs=None, info=None, wait_torch=True):
        """ac3mi_frame_scan_batch: streams [S][stride] u8 on the device (stride a multiple of 16, base 16-byte aligned), lens
        int32 / uint32 [S] on the device (stream s is streams[s, :lens[s]]) -> (refs u8 [S][max_frames][8], info u8 [S][24]);
        `.cpu().numpy().view(capi.frame_ref_dtype())[..., 0]` and `.view(capi.scan_info_dtype())[..., 0]` name the fields.
        Entries of refs at or behind a stream's n_frames keep what they held (zeros in a tensor allocated here)."""
        import torch
        assert streams.dtype == torch.uint8 and streams.is_contiguous() and streams.is_cuda and streams.dim() == 2
        S, stride = streams.shape
        assert lens.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and lens.is_contiguous() and lens.is_cuda and lens.numel() == S
        if refs is None:
            refs = torch.zeros((S, int(max_frames), 8), dtype=torch.uint8, device=streams.device)
        if info is None:
            info = torch.zeros((S, 24), dtype=torch.uint8, device=streams.device)
        assert refs.dtype == torch.uint8 and refs.is_contiguous() and refs.numel() == S * int(max_frames) * 8
        assert info.dtype == torch.uint8 and info.is_contiguous() and info.numel() == S * 24
        self._drain_torch(wait_torch)
        self._check(self.lib.ac3mi_frame_scan_batch(ctypes.c_void_p(self.ctx), ctypes.c_void_p(streams.data_ptr()), ctypes.c_size_t(stride),
                                                    ctypes.c_void_p(lens.data_ptr()), int(S), int(mode), int(max_frames),
                                                    ctypes.c_void_p(refs.data_ptr()), ctypes.c_void_p(info.data_ptr())))
        self._keep.append((streams, lens, refs, info))
        return refs, info

    def frame_gather_batch(self, streams, refs, info, frames_per_stream, frame_bytes, first_frame=0, frame_stride=None, out=None,
                           wait_torch=True):
        """ac3mi_frame_gather_batch: the frames first_frame .. first_frame + frames_per_stream - 1 of every stream of a
        frame_scan_batch (its streams [S][stride], refs and info) -> frames u8 [S][frames_per_stream][frame_stride] (default:
        frame_bytes rounded up to 16), as decode_batch / decode_s16_batch / transcode_batch take them; a slot without a frame,
        or whose frame is longer than frame_bytes, is all zeros."""
        import torch
        assert streams.dtype == torch.uint8 and streams.is_contiguous() and streams.is_cuda and streams.dim() == 2
        S, stride = streams.shape
        assert refs.dtype == torch.uint8 and refs.is_contiguous() and refs.dim() == 3 and refs.shape[0] == S and refs.shape[2] == 8
        assert info.dtype == torch.uint8 and info.is_contiguous() and info.numel() == S * 24
        if frame_stride is None:
            frame_stride = (int(frame_bytes) + 15) & ~15
        if out is None:
            out = torch.empty((S, int(frames_per_stream), int(frame_stride)), dtype=torch.uint8, device=streams.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == S * int(frames_per_stream) * int(frame_stride)
        self._drain_torch(wait_torch)
        self._check(self.lib.ac3mi_frame_gather_batch(ctypes.c_void_p(self.ctx), ctypes.c_void_p(streams.data_ptr()), ctypes.c_size_t(stride),
                                                      int(S), ctypes.c_void_p(refs.data_ptr()), ctypes.c_void_p(info.data_ptr()),
                                                      int(refs.shape[1]), int(first_frame), int(frames_per_stream),
                                                      ctypes.c_void_p(out.data_ptr()), int(frame_stride), int(frame_bytes)))
        self._keep.append((streams, refs, info, out))
        return out

    def _pcm_call(self, pcm, state_bytes_entry, state):
        """What every PCM tool takes: pcm [S][F][1536][channels] s16 on the device and state u8 [S][state bytes] (None: zeros,
        allocated here) -> (S, F, channels, state)"""
        import torch
        assert pcm.dtype == torch.int16 and pcm.is_contiguous() and pcm.is_cuda and pcm.dim() == 4 and pcm.shape[2] == 1536
        S, F, _, nch = pcm.shape
        nb = int(getattr(self.lib, state_bytes_entry)())
        if state is None:
            state = torch.zeros((S, nb), dtype=torch.uint8, device=pcm.device)
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() == S * nb
        return S, F, nch, state

    def _launch(self, wait_torch, entry, keep, *args):
        """entry(ctx, *args) behind torch's queued work; `keep` stays referenced until the next sync"""
        self._drain_torch(wait_torch)
        self._check(getattr(self.lib, entry)(ctypes.c_void_p(self.ctx), *args))
        self._keep.append(keep)

    def _read_batch(self, entry, state_bytes, ResultC, state, out, wait_torch, *extra):
        """A PCM tool's device read-out: state u8 [S][state bytes], then `extra`, -> results u8 [S][sizeof(ResultC)]"""
        import torch
        nb, nr = int(getattr(self.lib, state_bytes)()), ctypes.sizeof(ResultC)
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.is_cuda and state.numel() % nb == 0
        S = state.numel() // nb
        if out is None:
            out = torch.zeros((S, nr), dtype=torch.uint8, device=state.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == S * nr
        self._launch(wait_torch, entry, (state, out), ctypes.c_void_p(state.data_ptr()), int(S), *extra, ctypes.c_void_p(out.data_ptr()))
        return out

    def loudness_batch(self, sample_rate, roles, pcm, state=None, wait_torch=True):
        """ac3mi_loudness_batch: meters pcm [S][F][1536][channels] s16 on the device (any 2-byte aligned view that is
        contiguous) into state u8 [S][loudness_state_bytes()] (zeros: new streams; default: allocated here) -> state.  roles:
        one of 0 / 1 / 2 per channel (loudness_roles)."""
        S, F, nch, state = self._pcm_call(pcm, "ac3mi_loudness_state_bytes", state)
        desc = capi.LoudnessDescC(int(sample_rate), int(nch), _roles_array(roles, nch))
        self._launch(wait_torch, "ac3mi_loudness_batch", (pcm, state), ctypes.byref(desc), ctypes.c_void_p(pcm.data_ptr()), int(S), int(F),
                     ctypes.c_void_p(state.data_ptr()))
        return state

    def loudness_read_batch(self, state, out=None, wait_torch=True):
        """ac3mi_loudness_read_batch: state u8 [S][loudness_state_bytes()] -> results u8 [S][40];
        `.cpu().numpy().view(capi.loudness_result_dtype())[..., 0]` names the fields."""
        return self._read_batch("ac3mi_loudness_read_batch", "ac3mi_loudness_state_bytes", capi.LoudnessResultC, state, out, wait_torch)

    def loudness_range_batch(self, sample_rate, roles, pcm, state=None, range_state=None, wait_torch=True):
        """ac3mi_loudness_range_batch: loudness_batch and the EBU Tech 3342 range meter in one pass over pcm -> (state,
        range_state); range_state u8 [S][loudness_range_state_bytes()] belongs to the state it was started with (zeros: new
        streams; default: allocated here, both together)."""
        import torch
        if (state is None) != (range_state is None):
            raise ValueError("a range state belongs to the loudness state it was started with: pass both or neither")
        S, F, nch, state = self._pcm_call(pcm, "ac3mi_loudness_state_bytes", state)
        nr = int(self.lib.ac3mi_loudness_range_state_bytes())
        if range_state is None:
            range_state = torch.zeros((S, nr), dtype=torch.uint8, device=pcm.device)
        assert range_state.dtype == torch.uint8 and range_state.is_contiguous() and range_state.is_cuda and range_state.numel() == S * nr
        desc = capi.LoudnessDescC(int(sample_rate), int(nch), _roles_array(roles, nch))
        self._launch(wait_torch, "ac3mi_loudness_range_batch", (pcm, state, range_state), ctypes.byref(desc), ctypes.c_void_p(pcm.data_ptr()),
                     int(S), int(F), ctypes.c_void_p(state.data_ptr()), ctypes.c_void_p(range_state.data_ptr()))
        return state, range_state

    def loudness_range_read_batch(self, range_state, out=None, wait_torch=True):
        """ac3mi_loudness_range_read_batch: range_state u8 [S][loudness_range_state_bytes()] -> results u8 [S][48];
        `.cpu().numpy().view(capi.loudness_range_result_dtype())[..., 0]` names the fields."""
        return self._read_batch("ac3mi_loudness_range_read_batch", "ac3mi_loudness_range_state_bytes", capi.LoudnessRangeResultC, range_state,
                                out, wait_torch)

    def loudness_words_batch(self, results, frames_per_stream, base_word, out=None, wait_torch=True):
        """ac3mi_loudness_words_batch: results u8 [S][40] (loudness_read_batch) -> words int32 [S][frames_per_stream], base_word
        with each stream's dialnorm (base_word's own where a stream is flagged empty), for set_encode_metadata_frames."""
        import torch
        nr = ctypes.sizeof(capi.LoudnessResultC)
        assert results.dtype == torch.uint8 and results.is_contiguous() and results.is_cuda and results.numel() % nr == 0
        S = results.numel() // nr
        if out is None:
            out = torch.zeros((S, int(frames_per_stream)), dtype=torch.int32, device=results.device)
        assert out.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and out.is_contiguous() and out.numel() == S * int(frames_per_stream)
        self._launch(wait_torch, "ac3mi_loudness_words_batch", (results, out), ctypes.c_void_p(results.data_ptr()), int(S),
                     int(frames_per_stream), ctypes.c_uint32(int(base_word) & 0xffffffff), ctypes.c_void_p(out.data_ptr()))
        return out

    def truepeak_batch(self, roles, pcm, state=None, wait_torch=True):
        """ac3mi_truepeak_batch: meters pcm [S][F][1536][channels] s16 on the device (any 2-byte aligned view that is
        contiguous) into state u8 [S][truepeak_state_bytes()] (zeros: new streams; default: allocated here) -> state.  roles:
        0 = not measured, anything else = measured, one per channel (loudness_roles' list can be passed as it is)."""
        S, F, nch, state = self._pcm_call(pcm, "ac3mi_truepeak_state_bytes", state)
        self._launch(wait_torch, "ac3mi_truepeak_batch", (pcm, state), int(nch), _roles_array(roles, nch), ctypes.c_void_p(pcm.data_ptr()),
                     int(S), int(F), ctypes.c_void_p(state.data_ptr()))
        return state

    def truepeak_read_batch(self, state, ceiling_q28=0, out=None, wait_torch=True):
        """ac3mi_truepeak_read_batch: state u8 [S][truepeak_state_bytes()] -> results u8 [S][96];
        `.cpu().numpy().view(capi.truepeak_result_dtype())[..., 0]` names the fields.  ceiling_q28: truepeak_ceiling(dBTP), 0 = none."""
        return self._read_batch("ac3mi_truepeak_read_batch", "ac3mi_truepeak_state_bytes", capi.TruePeakResultC, state, out, wait_torch,
                                ctypes.c_uint32(int(ceiling_q28)))

    def limit_batch(self, roles, ceiling_q28, release_step_q24, pcm, state=None, out=None, wait_torch=True):
        """ac3mi_limit_batch: limits pcm [S][F][1536][channels] s16 on the device to ceiling_q28 (truepeak_ceiling(dBTP)) with
        release step release_step_q24 (limit_release_step) -> (out, state).  out: the same shape (default: allocated here;
        `pcm` itself: in place); state u8 [S][limit_state_bytes()] (zeros: new streams; default: allocated here).  roles: 0 =
        not detected, anything else = detected; every channel is delayed by 77 samples and gets the stream's gain."""
        import torch
        S, F, nch, state = self._pcm_call(pcm, "ac3mi_limit_state_bytes", state)
        if out is None:
            out = torch.empty_like(pcm)
        assert out.dtype == torch.int16 and out.is_contiguous() and out.is_cuda and out.numel() == pcm.numel()
        self._launch(wait_torch, "ac3mi_limit_batch", (pcm, out, state), int(nch), _roles_array(roles, nch), ctypes.c_uint32(int(ceiling_q28)),
                     ctypes.c_uint32(int(release_step_q24)), ctypes.c_void_p(pcm.data_ptr()), ctypes.c_void_p(out.data_ptr()), int(S), int(F),
                     ctypes.c_void_p(state.data_ptr()))
        return out, state

    def limit_read_batch(self, state, out=None, wait_torch=True):
        """ac3mi_limit_read_batch: state u8 [S][limit_state_bytes()] -> results u8 [S][40];
        `.cpu().numpy().view(capi.limit_result_dtype())[..., 0]` names the fields."""
        return self._read_batch("ac3mi_limit_read_batch", "ac3mi_limit_state_bytes", capi.LimitResultC, state, out, wait_torch)

    def resample_batch(self, desc, pcm, out_frames, state=None, out=None, status=None, wait_torch=True):
        """ac3mi_resample_batch: converts pcm [S][F][1536][channels] s16 on the device from desc.in_rate to desc.out_rate ->
        (out [S][out_frames][1536][channels], state, status).  out_frames is what resample_plan gives for the streams' age;
        state u8 [S][resample_state_bytes()] (zeros: new streams; default: allocated here); status u32 [S]: 0, or why a
        stream was left untouched with zeros for output.  desc: a ResampleDesc or (in_rate, out_rate)."""
        import torch
        S, F, nch, state = self._pcm_call(pcm, "ac3mi_resample_state_bytes", state)
        if not isinstance(desc, capi.ResampleDescC):
            desc = capi.ResampleDescC(int(desc[0]), int(desc[1]), int(nch))
        if desc.channels != nch:
            raise ValueError("desc.channels is pcm's last dimension")
        if out is None:
            out = torch.empty((S, int(out_frames), 1536, nch), dtype=torch.int16, device=pcm.device)
        if status is None:
            status = torch.zeros((S,), dtype=torch.int32, device=pcm.device)
        assert out.dtype == torch.int16 and out.is_contiguous() and out.is_cuda and out.numel() == S * int(out_frames) * 1536 * nch
        assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() == S
        self._launch(wait_torch, "ac3mi_resample_batch", (pcm, out, state, status), ctypes.byref(desc), ctypes.c_void_p(pcm.data_ptr()), int(S),
                     int(F), ctypes.c_void_p(out.data_ptr()) if out.numel() else None, int(out_frames), ctypes.c_void_p(state.data_ptr()),
                     ctypes.c_void_p(status.data_ptr()))
        return out, state, status

    def set_encode_drc(self, profile, state=None):
        """Dynamic range control (ac3mi_set_encode_drc): profile 0 = no dynrng words, 1..5 = film standard / film light /
        music standard / music light / speech; `state` int32 [S] on the device (the smoothing state, indexed like
        csnroffst, 0 for new streams, updated in place; kept referenced while set).  Applies to encode_batch and
        transcode_batch."""
        if state is not None:
            import torch
            if state.dtype != torch.int32 or not state.is_cuda or not state.is_contiguous():
                raise ValueError("state must be a contiguous int32 tensor on the device")
        ptr = ctypes.c_void_p(state.data_ptr()) if state is not None else None
        self._check(self.lib.ac3mi_set_encode_drc(ctypes.c_void_p(self.ctx), int(profile), ptr))
        self._drc_state = state if int(profile) else None

    def set_encode_dynrng_frames(self, dynrng=None, compr=None):
        """Dynamic range words per frame (ac3mi_set_encode_dynrng_frames): `dynrng` uint8 [S][F][6][2] on the device, the
        dynrng word in force in each block for programme 0 / 1 (a block sends when its word differs from the block before it,
        block 0 when it is not 0); `compr` int16 / uint16 [S][F][2], bit 8 compre, bits 0-7 the word.  Both by the frame's
        position in the following encode_batch / transcode_batch calls (kept referenced while set); None: none."""
        import torch
        if dynrng is not None and (dynrng.dtype != torch.uint8 or not dynrng.is_cuda or not dynrng.is_contiguous()):
            raise ValueError("dynrng must be a contiguous uint8 tensor on the device")
        if compr is not None and (compr.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or not compr.is_cuda
                                  or not compr.is_contiguous()):
            raise ValueError("compr must be a contiguous int16 / uint16 tensor on the device")
        if dynrng is not None or compr is not None:
            torch.cuda.current_stream().synchronize()       # their fill was queued on torch's stream
        self._check(self.lib.ac3mi_set_encode_dynrng_frames(ctypes.c_void_p(self.ctx),
                                                            ctypes.c_void_p(dynrng.data_ptr()) if dynrng is not None else None,
                                                            ctypes.c_void_p(compr.data_ptr()) if compr is not None else None))
        self._dyn_words = (dynrng, compr)

    def set_encode_drc_source(self, mode):
        """Where transcode_batch takes the new frames' dynrng and compr words from (ac3mi_set_encode_drc_source): 0 = the
        context's settings, 1 = each source frame's own words (flags.DRC_SOURCE_FOLLOW; the decode descriptor must have
        dynrng 0).  Meant to be used together with set_encode_metadata_source(1): the words are relative to dialnorm."""
        self._check(self.lib.ac3mi_set_encode_drc_source(ctypes.c_void_p(self.ctx), int(mode)))

    def set_encode_exp_strategy(self, mode):
        """Exponent strategies (ac3mi_set_encode_exp_strategy): 0 = the reference's rule, 1 = the partition of each frame's
        six blocks into exponent sets that costs the fewest bits under the header's model.  Applies to encode_batch and
        transcode_batch."""
        self._check(self.lib.ac3mi_set_encode_exp_strategy(ctypes.c_void_p(self.ctx), int(mode)))

    def set_encode_layout(self, mode, acmod=None, lfeon=0):
        """Channel layout of the encoded frames (ac3mi_set_encode_layout): 0 = the reference's table by channel count, 1 = code
        `acmod` (0..7) with `lfeon` (0/1) - channels must then be nfchans(acmod) + lfeon, coded in A/52's order with the
        LFE last -, 2 = transcode_batch codes the layout the decoder granted (chmap not read; encode_batch codes as mode 0).
        Applies to encode_batch and transcode_batch."""
        self._check(self.lib.ac3mi_set_encode_layout(ctypes.c_void_p(self.ctx), int(mode), -1 if acmod is None else int(acmod),
                                                     int(lfeon)))

    def set_mix_state(self, pending=None, flags=None):
        """liba52's overlap bookkeeping around frames with surround level 0 (ac3mi_set_mix_state): `pending` float32 shaped
        like the delay array, `flags` int32 [S][6], both zero for new streams and updated in place by the decode calls that
        follow; None, None returns to the plain linear mix.  The tensors must stay alive while set."""
        if (pending is None) != (flags is None):
            raise ValueError("set_mix_state: give both arrays or neither")
        if pending is not None:
            import torch
            assert pending.dtype == torch.float32 and flags.dtype == torch.int32 and pending.is_cuda and flags.is_cuda
            torch.cuda.current_stream().synchronize()        # their zero fill was queued on torch's stream
        self._mix_state = (pending, flags)
        self._check(self.lib.ac3mi_set_mix_state(ctypes.c_void_p(self.ctx),
                                                 ctypes.c_void_p(pending.data_ptr() if pending is not None else 0),
                                                 ctypes.c_void_p(flags.data_ptr() if flags is not None else 0)))

    def transcode_batch(self, dec, enc, frames, delay, lfsr, chmap, last, csnroffst, out=None, status=None, wait_torch=True):
        """frames [S][F][in_stride] u8 -> re-encoded frames [S][F][out_stride] u8 (+ status [S][F]); the state arrays
        are those of decode_batch (delay, lfsr) and encode_batch (last, csnroffst), all updated in place."""
        import torch
        S, F, in_stride = frames.shape
        fb = enc.frame_bytes()
        stride = (fb + 3) & ~3
        dev = frames.device
        if out is None:
            out = torch.zeros((S, F, stride), dtype=torch.uint8, device=dev)
        if status is None:
            status = torch.zeros((S, F), dtype=torch.int32, device=dev)
        cm = (ctypes.c_uint8 * 8)(*(list(chmap) + [0] * 8)[:8]) if chmap is not None else None
        dc, ec = dec.c(), enc.c()
        self._drain_torch(wait_torch)
        self._check(self.lib.ac3mi_transcode_batch(self.ctx, ctypes.byref(dc), ctypes.byref(ec), frames.data_ptr(), in_stride, S, F,
                                                   delay.data_ptr(), lfsr.data_ptr(), cm, last.data_ptr(), csnroffst.data_ptr(),
                                                   out.data_ptr(), stride, status.data_ptr()))
        self._keep.append((frames, delay, lfsr, last, csnroffst, out, status))
        return out, status

    def encode_batch(self, desc, pcm, chmap, last, csnroffst, out=None, taps=False, wait_torch=True):
        """pcm [S][F][1536][nch] s16, chmap = nch ints, last [S][nch][256] s16, csnroffst [S] i32 (both
        updated in place) -> frames [S][F][stride] u8 (stride = frame bytes rounded up to 4)[, taps dict]."""
        import torch
        fb = desc.frame_bytes()
        if fb <= 0:
            raise capi.AC3MIError("AC3_encode_init would reject %r" % (desc,))
        S, F, n, nch = pcm.shape
        assert n == 1536 and nch == desc.channels and pcm.dtype == torch.int16 and pcm.is_contiguous() and pcm.is_cuda
        assert last.dtype == torch.int16 and tuple(last.shape) == (S, nch, 256) and last.is_contiguous()
        assert csnroffst.dtype == torch.int32 and tuple(csnroffst.shape) == (S,)
        stride = (fb + 3) & ~3
        dev = pcm.device
        if out is None:
            out = torch.zeros((S, F, stride), dtype=torch.uint8, device=dev)
        else:
            assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape[:2] == (S, F) and out.shape[2] >= stride and out.shape[2] % 4 == 0
            stride = out.shape[2]
        cm = (ctypes.c_uint8 * 8)(*(list(chmap) + [0] * 8)[:8])
        tp, tdict = None, None
        if taps:
            tdict = {
                "mdct": torch.zeros((S, F, 6, nch, 256), dtype=torch.int32, device=dev),
                "exponent": torch.zeros((S, F, 6, nch, 256), dtype=torch.uint8, device=dev),
                "exp_samples": torch.zeros((S, F, 6, nch), dtype=torch.int8, device=dev),
                "encoded_exp": torch.zeros((S, F, 6, nch, 256), dtype=torch.uint8, device=dev),
                "bap": torch.zeros((S, F, 6, nch, 256), dtype=torch.uint8, device=dev),
                "exp_strategy": torch.zeros((S, F, 6, nch), dtype=torch.uint8, device=dev),
                "snroffst": torch.zeros((S, F, 2), dtype=torch.int32, device=dev),
            }
            tp = capi.EncodeTapsC(*(tdict[k].data_ptr() for k in ("mdct", "exponent", "exp_samples", "encoded_exp",
                                                                   "bap", "exp_strategy", "snroffst")))
        c = desc.c()
        self._drain_torch(wait_torch or taps)
        self._check(self.lib.ac3mi_encode_batch(self.ctx, ctypes.byref(c), pcm.data_ptr(), cm, last.data_ptr(),
                                                csnroffst.data_ptr(), out.data_ptr(), stride, S, F,
                                                ctypes.byref(tp) if tp else None))
        self._keep.append((pcm, last, csnroffst, out, tdict))
        if taps:
            return out, tdict
        return out
