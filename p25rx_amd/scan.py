"""The survey of docs/SPEC.md 3.0h (p25fe_scan_t): the per-bin power spectrum of ONE capture row of any rate, summed as integers on
the GPU (kernel k_scan), and the list of active raster channels formed from it on the host.  It is the stage in front of the tuner:

    sc = Scanner(fe, N=4096, hop=2048)
    acc = sc.scan_dev(capture)                                 # uint64 [N + 1] on the device, added into
    for ch in Scanner.channels(acc.cpu().numpy(), fs):         # strongest first
        step = Tuner.nco_step(fs, ch["centre_hz"] + ch["offset_hz"])

and, with a time axis (3.0i: kernel k_waterfall, one launch for all slots), which raster channel was keyed from when to when:

    rows = sc.waterfall_dev(capture, B=12)                     # int64 [n_slots, N + 1] on the device: one record per slot of B frames
    for k in Scanner.keys(rows.cpu().numpy(), fs):             # by first slot: raster_index, first_slot, n_slots, offset_hz, ...

and the same keys without the rows leaving the device (3.0k: three kernels and a memset, the same bytes as Scanner.keys):

    kp = sc.keys_plan(fs, max_rows=256, max_keys=64)
    kp.run_dev(rows)                                           # behind waterfall_dev on the same stream; synchronises nothing
    for k in kp.read():                                        # waits for the run; only the keys cross the bus

torch supplies device memory and streams only; all arithmetic on the samples happens in libp25fe.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FMT_CF32, FMT_U8, FMT_S16, SCAN_CHAN_DTYPE, WATERFALL_KEY_DTYPE


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Scanner:
    """A survey object made for one FrontEnd (its device and u8 conversion; its channel count does not matter), which must outlive
    it.  N is 1024 or 4096, hop a multiple of 8 that divides N, window N real values (None: the designed periodic Hann)."""

    @staticmethod
    def design(N):
        """the designed window, float32 [N] (p25fe_scan_window; needs no device)"""
        L_ = _lib.load()
        w = np.empty(max(int(N), 0), dtype=np.float32)
        _lib.check(L_, None, L_.p25fe_scan_window(int(N), _p(w), w.size))
        return w

    @staticmethod
    def n_frames(hop, abs0, n):
        """frames the range [abs0, abs0 + n) owns: those whose last sample f * hop + hop - 1 lies in it"""
        return (int(abs0) + int(n)) // int(hop) - int(abs0) // int(hop)

    @staticmethod
    def channels(acc, fs_hz, raster_hz=12500.0, half_bw_hz=4000.0, thr_db=20.0, cap=None):
        """a record on the host (uint64 [N + 1]) -> the active raster channels, strongest first, as a structured array of
        SCAN_CHAN_DTYPE (p25fe_scan_channels; needs no device).  cap limits how many are returned, not how many are counted:
        with cap the result is (channels, n_active)."""
        L_ = _lib.load()
        acc = np.ascontiguousarray(acc, dtype=np.uint64)
        N = acc.size - 1
        n = C.c_size_t(0)
        want = N if cap is None else int(cap)
        out = np.zeros(max(want, 1), dtype=SCAN_CHAN_DTYPE)
        _lib.check(L_, None, L_.p25fe_scan_channels(_p(acc), N, int(fs_hz), float(raster_hz), float(half_bw_hz), float(thr_db),
                                                    _p(out), want, C.byref(n)))
        got = out[:min(n.value, want)].copy()
        return got if cap is None else (got, n.value)

    @staticmethod
    def slots(hop, B, abs0, n):
        """the slots of B frames the frames of [abs0, abs0 + n) fall into -> (first_slot, n_slots); n_slots = 0 when the range owns
        no frame (p25fe_waterfall_slots; needs no device)"""
        L_ = _lib.load()
        first, cnt = C.c_uint64(0), C.c_size_t(0)
        _lib.check(L_, None, L_.p25fe_waterfall_slots(int(hop), int(B), int(abs0), int(n), C.byref(first), C.byref(cnt)))
        return first.value, cnt.value

    @staticmethod
    def keys(rows, fs_hz, slot0=0, raster_hz=12500.0, half_bw_hz=4000.0, on_db=20.0, off_db=14.0, min_slots=2, cap=None, N=None):
        """rows on the host (uint64 or int64 words [n_rows, row_stride]; N: row_stride - 1 unless given, the rest of a row is
        padding) -> the keyed intervals by first slot, then raster index, as a structured array of WATERFALL_KEY_DTYPE
        (p25fe_waterfall_keys; needs no device).  With cap the result is (keys, n_intervals)."""
        L_ = _lib.load()
        rows = np.ascontiguousarray(rows)
        rows = rows.view(np.uint64) if rows.dtype == np.int64 else rows.astype(np.uint64, copy=False)
        assert rows.ndim == 2
        stride = rows.shape[1]
        N = stride - 1 if N is None else int(N)
        n = C.c_size_t(0)
        want = 64 if cap is None else int(cap)
        while True:
            out = np.zeros(max(want, 1), dtype=WATERFALL_KEY_DTYPE)
            _lib.check(L_, None, L_.p25fe_waterfall_keys(_p(rows), rows.shape[0], stride, N, int(fs_hz), int(slot0), float(raster_hz),
                                                         float(half_bw_hz), float(on_db), float(off_db), int(min_slots), _p(out),
                                                         want, C.byref(n)))
            if cap is not None or n.value <= want:
                break
            want = n.value
        got = out[:min(n.value, want)].copy()
        return got if cap is None else (got, n.value)

    def __init__(self, fe, N=4096, hop=None, window=None, shift=16):
        self.fe, self.lib = fe, fe.L
        self.N, self.hop, self.shift = int(N), int(N) // 2 if hop is None else int(hop), int(shift)
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float32)
            if window.size != self.N:
                raise _lib.P25feError(_lib.ERR_ARG, "the window holds N values")
        self.sc = C.c_void_p()
        _lib.check(self.lib, fe.h, self.lib.p25fe_scan_create(fe.h, self.N, self.hop, None if window is None else _p(window),
                                                              self.shift, C.byref(self.sc)))

    def close(self):
        if getattr(self, "sc", None):
            self.lib.p25fe_scan_destroy(self.sc)
            self.sc = None

    __del__ = close

    def reset(self):
        """the host streaming form starts over, with a zeroed record"""
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_scan_reset(self.sc))

    def scan_dev(self, iq, n_hist=0, abs0=0, offset=0, n=None, acc=None):
        """cf32, int16 or uint8 [n, 2] on the device -> the record, uint64 [N + 1] on the device (torch has no uint64 arithmetic:
        an int64 tensor holds the words).  ADDS into `acc` (None: a zeroed one); `offset` = index of the first owned sample inside
        `iq` (>= n_hist), abs0 its position in the stream, n the owned samples (None: the rest of iq)."""
        import torch
        from .frontend import _torch_fmt, fmt_bytes
        assert iq.is_cuda and iq.dim() == 2 and iq.shape[1] == 2 and iq.is_contiguous()
        fmt = _torch_fmt(iq.dtype)
        if n is None:
            n = iq.shape[0] - offset
        assert 0 <= n <= iq.shape[0] - offset and 0 <= n_hist <= offset
        if acc is None:
            acc = torch.zeros(self.N + 1, dtype=torch.int64, device=iq.device)
        assert acc.is_cuda and acc.dtype == torch.int64 and acc.numel() >= self.N + 1 and acc.is_contiguous()
        _lib.check(self.lib, self.fe.h,
                   self.lib.p25fe_scan_dev(self.sc, C.c_void_p(iq.data_ptr() + fmt_bytes(fmt) * offset), fmt, n_hist, n, abs0,
                                           C.c_void_p(acc.data_ptr()), self.fe._stream()))
        return acc

    def scan(self, iq):
        """host streaming form: the capture's next samples (complex64 [n], int16 or uint8 interleaved pairs [2 n]) are added to the
        object's own record; the object keeps the history and the position between calls"""
        iq, fmt, n = self._host_samples(iq)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_scan(self.sc, _p(iq), fmt, n))

    @staticmethod
    def _host_samples(iq):
        """complex64 [n], int16 or uint8 interleaved pairs [2 n] -> (contiguous flat array, format, n)"""
        iq = np.asarray(iq)
        if iq.dtype == np.uint8:
            fmt = FMT_U8
        elif iq.dtype == np.int16:
            fmt = FMT_S16
        else:
            fmt, iq = FMT_CF32, iq.astype(np.complex64, copy=False)
        iq = np.ascontiguousarray(iq).reshape(-1)
        return iq, fmt, iq.size if fmt == FMT_CF32 else iq.size // 2

    def read(self, clear=False):
        """waits for the device and returns the object's record, uint64 [N + 1] (word N: the frames); clear zeroes it afterwards"""
        acc = np.empty(self.N + 1, dtype=np.uint64)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_scan_read(self.sc, _p(acc), 1 if clear else 0))
        return acc

    def waterfall_dev(self, iq, B, n_hist=0, abs0=0, offset=0, n=None, rows=None, slot0=None):
        """scan_dev with a time axis: the frames of the range go into one row per slot of B frames, int64 [n_rows, N + 1] on the
        device, in ONE launch.  ADDS into `rows` ([n_rows, >= N + 1], row 0 standing for slot `slot0`; None: zeroed rows for
        exactly the slots the range touches, slot0 None: its first slot).  abs0 matters in full: frame f belongs to slot f // B."""
        import torch
        from .frontend import _torch_fmt, fmt_bytes
        assert iq.is_cuda and iq.dim() == 2 and iq.shape[1] == 2 and iq.is_contiguous()
        fmt = _torch_fmt(iq.dtype)
        if n is None:
            n = iq.shape[0] - offset
        assert 0 <= n <= iq.shape[0] - offset and 0 <= n_hist <= offset
        if rows is None or slot0 is None:
            first, cnt = self.slots(self.hop, B, abs0, n)
            if slot0 is None:
                slot0 = first
            if rows is None:
                rows = torch.zeros((first + cnt - slot0 if first + cnt > slot0 else 0, self.N + 1), dtype=torch.int64, device=iq.device)
        assert rows.is_cuda and rows.dtype == torch.int64 and rows.dim() == 2 and rows.stride(1) == 1
        if rows.shape[0] == 0:                                       # no row has no address: nothing to call with
            if self.slots(self.hop, B, abs0, n)[1]:
                raise _lib.P25feError(_lib.ERR_ARG, "the range owns a frame and there is no row")
            return rows
        ptr, stride = C.c_void_p(rows.data_ptr()), rows.stride(0) if rows.shape[0] > 1 else rows.shape[1]
        _lib.check(self.lib, self.fe.h,
                   self.lib.p25fe_waterfall_dev(self.sc, C.c_void_p(iq.data_ptr() + fmt_bytes(fmt) * offset), fmt, n_hist, n, abs0,
                                                int(B), int(slot0), ptr, rows.shape[0], stride, self.fe._stream()))
        return rows

    def keys_plan(self, fs_hz, raster_hz=12500.0, half_bw_hz=4000.0, on_db=20.0, off_db=14.0, min_slots=2, max_rows=1024, max_keys=1024):
        """a Keys object for this survey's N and device: Scanner.keys' rule with these parameters, run on the device over up to
        max_rows rows for up to max_keys intervals"""
        return Keys(self, fs_hz, raster_hz, half_bw_hz, on_db, off_db, min_slots, max_rows, max_keys)

    def open_waterfall(self, B, max_rows):
        """the host streaming form gets rows: [max_rows, N + 1] zeroed on the device, for slots of B frames from slot 0"""
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_waterfall_open(self.sc, int(B), int(max_rows)))

    def waterfall(self, iq):
        """host streaming form, as scan(): the capture's next samples go into the open rows; may be mixed with scan() on one
        stream, each call's frames going where that call sends them"""
        iq, fmt, n = self._host_samples(iq)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_waterfall(self.sc, _p(iq), fmt, n))

    def read_waterfall(self):
        """waits for the device and returns the rows touched so far, uint64 [ceil(frames / B), N + 1]"""
        n = C.c_size_t(0)
        rc = self.lib.p25fe_waterfall_read(self.sc, None, 0, C.byref(n))
        if rc != _lib.ERR_CAPACITY:
            _lib.check(self.lib, self.fe.h, rc)
        rows = np.zeros((n.value, self.N + 1), dtype=np.uint64)
        if n.value:
            _lib.check(self.lib, self.fe.h, self.lib.p25fe_waterfall_read(self.sc, _p(rows), n.value, C.byref(n)))
        return rows


class Keys:
    """Scanner.keys on the device (p25fe_keys_t, docs/SPEC.md 3.0k): the plan of one raster over a Scanner's N, which must outlive
    it.  A run enqueues four launches on the front end's stream and synchronises nothing; read() waits for the last run and returns
    the bytes Scanner.keys returns for the same rows and parameters."""

    def __init__(self, scanner, fs_hz, raster_hz=12500.0, half_bw_hz=4000.0, on_db=20.0, off_db=14.0, min_slots=2, max_rows=1024,
                 max_keys=1024):
        self.scanner, self.lib = scanner, scanner.lib
        self.max_rows, self.max_keys = int(max_rows), int(max_keys)
        self.kp = C.c_void_p()
        _lib.check(self.lib, scanner.fe.h,
                   self.lib.p25fe_keys_create(scanner.sc, int(fs_hz), float(raster_hz), float(half_bw_hz), float(on_db), float(off_db),
                                              int(min_slots), self.max_rows, self.max_keys, C.byref(self.kp)))

    def close(self):
        if getattr(self, "kp", None):
            self.lib.p25fe_keys_destroy(self.kp)
            self.kp = None

    __del__ = close

    def run_dev(self, rows, slot0=0, n_rows=None):
        """rows as waterfall_dev returns them (int64 [n, >= N + 1] on the device, row 0 standing for slot `slot0`; the stride is
        the tensor's; n_rows: the first so many, None: all) -> the object's result, replacing the previous one.  The rows are
        read, never written."""
        assert rows.is_cuda and rows.element_size() == 8 and rows.dim() == 2 and rows.stride(1) == 1
        n = rows.shape[0] if n_rows is None else int(n_rows)
        assert 0 <= n <= rows.shape[0]
        stride = rows.stride(0) if rows.shape[0] > 1 else rows.shape[1]
        _lib.check(self.lib, self.scanner.fe.h,
                   self.lib.p25fe_keys_dev(self.kp, C.c_void_p(rows.data_ptr()), n, stride, int(slot0), self.scanner.fe._stream()))

    def run_stream(self):
        """the same run over the rows of the scanner's open host-streaming waterfall touched so far, from slot 0"""
        _lib.check(self.lib, self.scanner.fe.h, self.lib.p25fe_keys_stream(self.kp))

    def read(self, cap=None):
        """waits for the last run -> its keyed intervals by first slot, then raster index, as a structured array of
        WATERFALL_KEY_DTYPE; with cap the first cap of them and the count, (keys, n_intervals).  A run that found more than
        max_keys intervals raises P25feError with status ERR_CAPACITY and the true count in its `count`."""
        n = C.c_size_t(0)
        want = self.max_keys if cap is None else int(cap)
        out = np.zeros(max(want, 1), dtype=WATERFALL_KEY_DTYPE)
        rc = self.lib.p25fe_keys_read(self.kp, _p(out), want, C.byref(n))
        if rc != _lib.OK:
            try:
                _lib.check(self.lib, self.scanner.fe.h, rc)
            except _lib.P25feError as e:
                e.count = n.value
                raise
        got = out[:min(n.value, want)].copy()
        return got if cap is None else (got, n.value)
