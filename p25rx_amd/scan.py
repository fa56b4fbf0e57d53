"""The survey of docs/SPEC.md 3.0h (p25fe_scan_t): the per-bin power spectrum of ONE capture row of any rate, summed as integers on
the GPU (kernel k_scan), and the list of active raster channels formed from it on the host.  It is the stage in front of the tuner:

    sc = Scanner(fe, N=4096, hop=2048)
    acc = sc.scan_dev(capture)                                 # uint64 [N + 1] on the device, added into
    for ch in Scanner.channels(acc.cpu().numpy(), fs):         # strongest first
        step = Tuner.nco_step(fs, ch["centre_hz"] + ch["offset_hz"])

torch supplies device memory and streams only; all arithmetic on the samples happens in libp25fe.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FMT_CF32, FMT_U8, FMT_S16, SCAN_CHAN_DTYPE


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
        iq = np.asarray(iq)
        if iq.dtype == np.uint8:
            fmt = FMT_U8
        elif iq.dtype == np.int16:
            fmt = FMT_S16
        else:
            fmt, iq = FMT_CF32, iq.astype(np.complex64, copy=False)
        iq = np.ascontiguousarray(iq).reshape(-1)
        n = iq.size if fmt == FMT_CF32 else iq.size // 2
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_scan(self.sc, _p(iq), fmt, n))

    def read(self, clear=False):
        """waits for the device and returns the object's record, uint64 [N + 1] (word N: the frames); clear zeroes it afterwards"""
        acc = np.empty(self.N + 1, dtype=np.uint64)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_scan_read(self.sc, _p(acc), 1 if clear else 0))
        return acc
