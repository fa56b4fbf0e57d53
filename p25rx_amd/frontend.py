"""Handle-level Python view of the C ABI (include/p25fe.h).

`FrontEnd` owns one p25fe_t.  Host-buffer methods take/return NumPy arrays and mirror the
per-chunk bodies of DemodTask::run (src/demod.rs:70-117) and RecvTask::run
(src/recv.rs:148-150).  `*_dev` methods take torch CUDA tensors -- torch supplies device
memory and streams only; all arithmetic happens in libp25fe.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FMT_CF32, FMT_U8, FMT_S16, RESULT_DTYPE, ANCHOR_DTYPE
CHZ_CHANNELS = 192                  # P25FE_CHZ_CHANNELS (include/p25fe_spec.h)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def fmt_bytes(fmt):
    """bytes per complex sample of an input format: what a sample offset into an IQ buffer is multiplied by"""
    return {FMT_CF32: 8, FMT_S16: 4, FMT_U8: 2}[fmt]


def _torch_fmt(dtype):
    import torch
    try:
        return {torch.float32: FMT_CF32, torch.uint8: FMT_U8, torch.int16: FMT_S16}[dtype]
    except KeyError:
        raise TypeError("IQ tensor must be float32, int16 or uint8") from None


class FrontEnd:
    def __init__(self, n_channels=1, device=0, decim_taps=None, chan_taps=None, symbol_clock=0, **spec):
        """spec: the other p25fe_config_t fields by name (specialize, fm_deviation_hz, fm_sample_rate_hz, fm_gain, u8_scale,
        u8_offset, u8_lut, decim_phase, avg_taps) -- the run-time arguments of the reference's constructors
        (src/demod.rs:50, 52, 54, 83)."""
        self.L = _lib.load()
        # symbol_clock 0: fixed stride (the reference's receiver), 1: SPEC 3.8b, 2: 3.8b + 3.8c in run_dev / run_dev_pipelined / slice_dev
        cfg = _lib.make_config(n_channels=n_channels, device=device, decim_taps=decim_taps, chan_taps=chan_taps,
                               symbol_clock=symbol_clock, **spec)
        self.symbol_clock = symbol_clock & 0xff                  # (without P25FE_CLOCK_CAUSAL_OK)
        self.cfg = cfg
        self.C = n_channels
        self.device = device
        self.h = C.c_void_p()
        rc = self.L.p25fe_create(C.byref(cfg), C.byref(self.h))
        if rc == _lib.ERR_JIT:
            raise _lib.P25feError(rc, self.L.p25fe_strerror(rc).decode() + ": " + _lib.specialize_log()[-2000:])
        _lib.check(self.L, None, rc)

    @property
    def kernel_variant(self):
        """0: the library's own immediate-coefficient kernels, 1: kernels specialised for this handle's numbers, 2: generic"""
        return int(self.L.p25fe_kernel_variant(self.h))

    def format_variant(self, fmt):
        """the same for one input format (p25fe_format_variant): s16 has no specialised kernels and runs the generic ones on
        a handle whose numbers are not the build's; raises P25feError(ERR_JIT) where the handle requires specialised ones"""
        rc = int(self.L.p25fe_format_variant(self.h, int(fmt)))
        if rc < 0:
            self._chk(rc)
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.p25fe_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        _lib.check(self.L, self.h, rc)

    # ---- streaming, host buffers -------------------------------------------------------------
    def _demod(self, fn, arr, n_units, n_samples, want_power):
        cap = n_samples // 5 + 2
        bb = np.empty((self.C, cap), dtype=np.float32)
        n_out = C.c_size_t(0)
        pw = np.zeros(self.C, dtype=np.float32)
        self._chk(fn(self.h, _p(arr), n_units, _p(bb), cap, C.byref(n_out), _p(pw) if want_power else None))
        out = bb[:, :n_out.value]
        out = out[0].copy() if self.C == 1 else out.copy()
        if want_power:
            return out, (float(pw[0]) if self.C == 1 else pw)
        return out

    def demod_u8(self, data, want_power=False):
        """One DemodTask::run loop body on interleaved u8 I/Q; data shape [n_bytes] or [C, n_bytes]."""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(self.C, -1)
        return self._demod(self.L.p25fe_demod_u8, data, data.shape[1], data.shape[1] // 2, want_power)

    def demod_cf32(self, iq, want_power=False):
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(self.C, -1)
        return self._demod(self.L.p25fe_demod_cf32, iq, iq.shape[1], iq.shape[1], want_power)

    def demod_s16(self, iq, want_power=False):
        """the same on interleaved int16 I/Q (FMT_S16); iq shape [2 n] / [n, 2] or [C, ...]"""
        iq = np.ascontiguousarray(iq, dtype=np.int16).reshape(self.C, -1)
        return self._demod(self.L.p25fe_demod_s16, iq, iq.shape[1] // 2, iq.shape[1] // 2, want_power)

    def slice(self, bb, sync_cap=None):
        """RecvTask sample loop on baseband; returns (dibits, sync_pos, sync_dibit) (lists per channel if C > 1)."""
        bb = np.ascontiguousarray(bb, dtype=np.float32).reshape(self.C, -1)
        n = bb.shape[1]
        cap = n // 6 + 2                                         # hard ceiling: re-anchors are at least 6 samples apart (n // 10 + 1 is the undisturbed lock)
        scap = sync_cap if sync_cap is not None else n // 6 + 2
        dib = np.empty((self.C, cap), dtype=np.uint8)
        spos = np.empty((self.C, scap), dtype=np.int64)
        sdib = np.empty((self.C, scap), dtype=np.uint64)
        nd = (C.c_size_t * self.C)()
        ns = (C.c_size_t * self.C)()
        self._chk(self.L.p25fe_slice(self.h, _p(bb), n, _p(dib), cap, nd, _p(spos), _p(sdib), scap, ns))
        outs = [(dib[c, :nd[c]].copy(), spos[c, :min(ns[c], scap)].copy(), sdib[c, :min(ns[c], scap)].copy())
                for c in range(self.C)]
        return outs[0] if self.C == 1 else outs

    def _run(self, fn, arr, n_units, n_samples):
        cap = n_samples // 30 + 4                                # hard ceiling of the baseband (n // 5) under back-to-back re-anchors
        dib = np.empty((self.C, cap), dtype=np.uint8)
        nd = (C.c_size_t * self.C)()
        self._chk(fn(self.h, _p(arr), n_units, _p(dib), cap, nd))
        outs = [dib[c, :nd[c]].copy() for c in range(self.C)]
        return outs[0] if self.C == 1 else outs

    def run_u8(self, data):
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(self.C, -1)
        return self._run(self.L.p25fe_run_u8, data, data.shape[1], data.shape[1] // 2)

    def run_cf32(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(self.C, -1)
        return self._run(self.L.p25fe_run_cf32, iq, iq.shape[1], iq.shape[1])

    def run_s16(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.int16).reshape(self.C, -1)
        return self._run(self.L.p25fe_run_s16, iq, iq.shape[1] // 2, iq.shape[1] // 2)

    def run_host_windows(self, iq, window=0, fmt=None):
        """p25fe_run_host_windows: a LONG host capture through the path as a pipeline of windows (H2D copy | kernels | dibits
        back).  iq: numpy array (pageable: staged by the library) or a CPU torch tensor (pinned: copied from directly) --
        complex64 / float32 pairs (cf32), int16 pairs (s16) or uint8 pairs (u8), [n] or [C, n].  Returns (dibits per channel, stats dict)."""
        if hasattr(iq, "data_ptr"):                                  # torch CPU tensor (possibly pinned)
            import torch
            assert not iq.is_cuda and iq.is_contiguous()
            by_type = FMT_U8 if iq.dtype == torch.uint8 else (FMT_S16 if iq.dtype == torch.int16 else FMT_CF32)
            n_el = iq.numel() // self.C
            n = n_el // 2
            ptr = C.c_void_p(iq.data_ptr())
        else:
            by_type = FMT_U8 if iq.dtype == np.uint8 else (FMT_S16 if iq.dtype == np.int16 else FMT_CF32)
            iq = np.ascontiguousarray(iq if by_type != FMT_CF32 else iq.view(np.float32) if iq.dtype == np.complex64 else iq.astype(np.float32))
            n = iq.size // self.C // 2
            ptr = _p(iq)
        fmt = by_type if fmt is None else fmt
        cap = n // 30 + 4
        dib = np.empty((self.C, cap), dtype=np.uint8)
        nd = (C.c_size_t * self.C)()
        st = _lib.WindowsStats()
        self._chk(self.L.p25fe_run_host_windows(self.h, ptr, fmt, n, int(window), _p(dib), cap, nd, C.byref(st)))
        outs = [dib[c, :nd[c]].copy() for c in range(self.C)]
        stats = dict(n_windows=int(st.n_windows), ms_total=st.ms_total, ms_h2d=st.ms_h2d, ms_compute=st.ms_compute,
                     pinned_input=bool(st.pinned_input))
        return (outs[0] if self.C == 1 else outs), stats

    def resync(self):
        self._chk(self.L.p25fe_resync(self.h))

    def reset(self):
        self._chk(self.L.p25fe_reset(self.h))

    def resync_at_dev(self, idx):
        """Lock drops for the NEXT receiver-running device call: idx = int64 device tensor [n] or [C, n] of ascending absolute
        baseband indices (lock is dropped before each); None / empty cancels.  The tensor is kept alive by the wrapper."""
        if idx is None or idx.numel() == 0:
            self._rs = None
            self._chk(self.L.p25fe_resync_at_dev(self.h, None, 0, 0))
            return
        import torch
        assert idx.is_cuda and idx.dtype == torch.int64 and idx.is_contiguous()
        if idx.dim() == 1:
            idx = idx.unsqueeze(0).expand(self.C, -1).contiguous() if self.C > 1 else idx.unsqueeze(0)
        assert idx.shape[0] == self.C
        self._rs = idx
        self._chk(self.L.p25fe_resync_at_dev(self.h, C.c_void_p(idx.data_ptr()), idx.shape[1], idx.stride(0)))

    def state_export(self):
        n = C.c_size_t(0)
        self._chk(self.L.p25fe_state_size(self.h, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        self._chk(self.L.p25fe_state_export(self.h, _p(buf), buf.size, C.byref(n)))
        return buf

    def state_import(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._chk(self.L.p25fe_state_import(self.h, _p(blob), blob.size))

    # ---- device-resident ranges (torch tensors as plumbing) -------------------------------------
    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _fmt_of(t):
        import torch
        return _torch_fmt(t.dtype), t.shape[-2] if t.dim() == 3 else t.shape[0]

    def _iq_view(self, iq):
        """iq: [n, 2] or [C, n, 2] contiguous per channel; returns (fmt, n, ch_stride)."""
        import torch
        assert iq.is_cuda and iq.shape[-1] == 2
        if iq.dim() == 2:
            iq = iq.unsqueeze(0)
        assert iq.shape[0] == self.C and iq.stride(2) == 1 and iq.stride(1) == 2
        fmt = _torch_fmt(iq.dtype)
        return fmt, iq.shape[1], (iq.stride(0) // 2 if self.C > 1 else iq.shape[1])

    @staticmethod
    def dibit_cap(n_iq):
        """Row size for the dibits of n_iq input samples: n / 50 plus proportional slack (200 ppm) for the transmitter's
        symbol clock, which a receiver that re-anchors on every sync word follows.  The row's stride is its capacity: the
        kernels never store past it and p25fe_result_t.n_dibits stays exact."""
        return (n_iq // 50 + n_iq // 250000 + 64 + 15) // 16 * 16

    def run_dev(self, iq, dibits=None, result=None):
        """Fresh-stream IQ -> dibits on device.  Returns (dibits[C, cap] uint8 cuda, result uint8 tensor)."""
        import torch
        fmt, n, stride = self._iq_view(iq)
        cap = self.dibit_cap(n)
        if dibits is None:
            dibits = torch.empty((self.C, cap), dtype=torch.uint8, device=iq.device)
        if result is None:
            result = torch.empty((self.C, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        self._chk(self.L.p25fe_run_dev(self.h, C.c_void_p(iq.data_ptr()), fmt, stride, n, C.c_void_p(dibits.data_ptr()),
                                       dibits.stride(0), C.c_void_p(result.data_ptr()), self._stream()))
        return dibits, result

    def run_dev_pipelined(self, iq, dibits=None, result=None):
        """run_dev for a sequence of captures: the receive kernels of this call overlap the next call's K1 (they run
        on a stream of the handle).  Outputs are complete after join_dev() + a synchronisation of the stream."""
        import torch
        fmt, n, stride = self._iq_view(iq)
        cap = self.dibit_cap(n)
        if dibits is None:
            dibits = torch.empty((self.C, cap), dtype=torch.uint8, device=iq.device)
        if result is None:
            result = torch.empty((self.C, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        self._chk(self.L.p25fe_run_dev_pipelined(self.h, C.c_void_p(iq.data_ptr()), fmt, stride, n,
                                                 C.c_void_p(dibits.data_ptr()), dibits.stride(0),
                                                 C.c_void_p(result.data_ptr()), self._stream()))
        # the receive kernels write these on the handle's own stream, which torch's caching allocator does not see: keep
        # the outputs of the calls still in flight alive even if the caller drops them (released by join_dev)
        self._inflight = (getattr(self, "_inflight", ()) + ((dibits, result),))[-2:]
        return dibits, result

    def join_dev(self):
        """the current stream waits for every receive kernel run_dev_pipelined has enqueued"""
        self._chk(self.L.p25fe_join_dev(self.h, self._stream()))
        self._inflight = ()

    def debug_planes(self, n_bb):
        """Diagnostic (p25fe_debug_planes_dev): the planar baseband and the sign words of the most recent scratch-using call, whose
        baseband length per channel was n_bb -> (float32 [C, n_floats], int32 [C, n_words]: the words' bits) device tensors, copied
        on the current stream.  Layout: PLPAD / planar_index in csrc/p25fe_kernels.hip."""
        import torch
        nf, nw = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.L.p25fe_debug_planes_size(self.h, int(n_bb), C.byref(nf), C.byref(nw)))
        dev = "cuda:%d" % self.device
        f = torch.empty((self.C, nf.value), dtype=torch.float32, device=dev)
        w = torch.empty((self.C, nw.value), dtype=torch.int32, device=dev)
        self._chk(self.L.p25fe_debug_planes_dev(self.h, int(n_bb), C.c_void_p(f.data_ptr()), f.stride(0), C.c_void_p(w.data_ptr()),
                                                w.stride(0), self._stream()))
        return f, w

    def demod_dev(self, iq, n_hist=0, abs0=0, bb=None, want_power=False, offset=0):
        """stages 1-5 on a device range; `offset` = index of the first owned sample inside `iq` (>= n_hist)."""
        import torch
        fmt, n_total, stride = self._iq_view(iq)
        n = n_total - offset
        nb = self.L.p25fe_n_baseband_h(self.h, abs0, n)
        if bb is None:
            bb = torch.empty((self.C, (nb + 7) // 4 * 4), dtype=torch.float32, device=iq.device)
        pw = torch.empty(self.C, dtype=torch.float32, device=iq.device) if want_power else None
        ptr = iq.data_ptr() + offset * fmt_bytes(fmt)
        self._chk(self.L.p25fe_demod_dev(self.h, C.c_void_p(ptr), fmt, stride, n_hist, n, abs0,
                                         C.c_void_p(bb.data_ptr()), bb.stride(0),
                                         C.c_void_p(pw.data_ptr()) if want_power else None, self._stream()))
        return (bb, nb, pw) if want_power else (bb, nb)

    def predecim_dev(self, iq, n_hist=0, abs0=0, offset=0, out=None):
        """Stage 0 (config 3): cf32, int16 or uint8 @ 2.4 Msps [n, 2] or [C, n, 2] -> cf32 @ 240 ksps [C, n_out, 2] on device."""
        import torch
        fmt, n_total, stride = self._iq_view(iq)
        n = n_total - offset
        no = self.L.p25fe_n_predecim(abs0, n)
        if out is None:
            out = torch.empty((self.C, (no + 3) // 2 * 2, 2), dtype=torch.float32, device=iq.device)
        if fmt != FMT_CF32:
            self._chk(self.L.p25fe_predecim_fmt_dev(self.h, C.c_void_p(iq.data_ptr() + fmt_bytes(fmt) * offset), fmt, stride, n_hist,
                                                    n, abs0, C.c_void_p(out.data_ptr()), out.stride(0) // 2, self._stream()))
            return out, no
        self._chk(self.L.p25fe_predecim_dev(self.h, C.c_void_p(iq.data_ptr() + 8 * offset), stride, n_hist, n, abs0,
                                            C.c_void_p(out.data_ptr()), out.stride(0) // 2, self._stream()))
        return out, no

    def channelise_dev(self, iq, n_hist=0, abs0=0, offset=0, out=None):
        """SPEC 3.11: wideband cf32, int16 or uint8 @ 2.4 Msps [n, 2] (device) -> [192, n_out (padded), 2] cf32 @ 240 ksps."""
        import torch
        assert iq.dim() == 2 and iq.shape[1] == 2
        fmt = _torch_fmt(iq.dtype)
        assert fmt == FMT_CF32 or (iq.is_cuda and iq.is_contiguous())
        n = iq.shape[0] - offset
        no = self.L.p25fe_n_predecim(abs0, n)
        if out is None:
            out = torch.empty((CHZ_CHANNELS, max(64, (no + 63) // 64 * 64), 2), dtype=torch.float32, device=iq.device)
        if fmt != FMT_CF32:
            self._chk(self.L.p25fe_channelise_fmt_dev(self.h, C.c_void_p(iq.data_ptr() + fmt_bytes(fmt) * offset), fmt, n_hist, n,
                                                      abs0, C.c_void_p(out.data_ptr()), out.stride(0) // 2, self._stream()))
            return out, no
        self._chk(self.L.p25fe_channelise_dev(self.h, C.c_void_p(iq.data_ptr() + 8 * offset), n_hist, n, abs0,
                                              C.c_void_p(out.data_ptr()), out.stride(0) // 2, self._stream()))
        return out, no

    def slice_dev(self, bb, n_bb, n_hist_bb=0, abs_bb0=0, anchor_in=None, offset=0, sync_cap=0):
        import torch
        dev = bb.device
        if bb.dim() == 1:
            bb = bb.unsqueeze(0)
        cap = (n_bb // 10 + 64 + 15) // 16 * 16
        dib = torch.empty((self.C, cap), dtype=torch.uint8, device=dev)
        res = torch.empty((self.C, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        spos = torch.empty((self.C, max(sync_cap, 1)), dtype=torch.int64, device=dev)
        sdib = torch.empty((self.C, max(sync_cap, 1)), dtype=torch.int64, device=dev)
        a_in = None
        if anchor_in is not None:
            a_in = torch.from_numpy(np.frombuffer(np.asarray(anchor_in, dtype=ANCHOR_DTYPE).tobytes(), dtype=np.uint8).copy()).to(dev)
        self._chk(self.L.p25fe_slice_dev(self.h, C.c_void_p(bb.data_ptr() + 4 * offset), bb.stride(0), n_hist_bb, n_bb,
                                         abs_bb0, C.c_void_p(a_in.data_ptr()) if a_in is not None else None,
                                         C.c_void_p(dib.data_ptr()), dib.stride(0),
                                         C.c_void_p(spos.data_ptr()) if sync_cap else None,
                                         C.c_void_p(sdib.data_ptr()) if sync_cap else None, sync_cap,
                                         C.c_void_p(res.data_ptr()), self._stream()))
        return dib, res, spos, sdib

    def nid_dev(self, dibits, n_dibits, sync_dibit, sync_pos=None, n_sync=None):
        """Network identifiers after the sync events of ONE channel: dibits uint8 [>= n_dibits], sync_dibit int64/uint64
        [n_sync] (device tensors) -> uint8 tensor [n_sync, 24] (view with _lib.NID_DTYPE after .cpu())."""
        import torch
        n_sync = int(sync_dibit.numel() if n_sync is None else n_sync)
        out = torch.empty((max(n_sync, 1), 24), dtype=torch.uint8, device=dibits.device)
        self._chk(self.L.p25fe_nid_dev(self.h, C.c_void_p(dibits.data_ptr()), int(n_dibits), C.c_void_p(sync_dibit.data_ptr()),
                                       C.c_void_p(sync_pos.data_ptr()) if sync_pos is not None else None, n_sync,
                                       C.c_void_p(out.data_ptr()), self._stream()))
        return out[:n_sync]

    def nid_batch_dev(self, dibits, results, sync_dibit, sync_pos=None):
        """Channel batch: dibits [C, dibit_stride] uint8, results uint8 [C, sizeof(p25fe_result_t)], sync_dibit /
        sync_pos [C, sync_stride] (all device tensors, as written by slice_dev) -> uint8 tensor [C, sync_stride, 24]
        (rows k >= results[c].n_sync are left untouched: zero)."""
        import torch
        sync_stride = sync_dibit.shape[1]
        out = torch.zeros((self.C, max(sync_stride, 1), 24), dtype=torch.uint8, device=dibits.device)
        self._chk(self.L.p25fe_nid_batch_dev(self.h, C.c_void_p(dibits.data_ptr()), dibits.stride(0),
                                             C.c_void_p(results.data_ptr()), C.c_void_p(sync_dibit.data_ptr()),
                                             C.c_void_p(sync_pos.data_ptr()) if sync_pos is not None else None,
                                             sync_stride, C.c_void_p(out.data_ptr()), self._stream()))
        return out[:, :sync_stride]

    def chan_stats_dev(self, results, nid=None, power_dbm=None):
        """results [C, sizeof(p25fe_result_t)], nid [C, sync_stride, 24] (optional), power_dbm [C] float32
        (optional) -> uint8 tensor [C, 64] (view with _lib.CHAN_STATS_DTYPE after .cpu())."""
        import torch
        out = torch.empty((self.C, 64), dtype=torch.uint8, device=results.device)
        self._chk(self.L.p25fe_chan_stats_dev(self.h, C.c_void_p(results.data_ptr()),
                                              C.c_void_p(nid.data_ptr()) if nid is not None else None,
                                              nid.shape[1] if nid is not None else 0,
                                              C.c_void_p(power_dbm.data_ptr()) if power_dbm is not None else None,
                                              C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def profile_enable(self, on=True):
        """True / 1: events around every kernel; 2: around K1 only; 3: around K1 on every 8th call; False / 0: off."""
        self._chk(self.L.p25fe_profile_enable(self.h, int(on)))

    def profile_read(self):
        """-> (ms per kernel [K1 front end, K2 sync, K3 scan, K4 slice] summed over calls, n_calls)."""
        ms = (C.c_double * 4)()
        n = C.c_uint64(0)
        self._chk(self.L.p25fe_profile_read(self.h, C.byref(ms), C.byref(n)))
        return [ms[i] for i in range(4)], n.value

    def n_baseband(self, abs0, n):
        """baseband samples n input samples from absolute index abs0 give, with THIS handle's decimator phase"""
        return int(self.L.p25fe_n_baseband_h(self.h, abs0, n))

    def shard_halo(self):
        return self.L.p25fe_shard_halo()

    def shard_pass1(self, iq, offset, n_hist, abs0, result=None):
        import torch
        fmt, n_total, stride = self._iq_view(iq)
        n = n_total - offset
        if result is None:
            result = torch.empty((self.C, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        ptr = iq.data_ptr() + offset * fmt_bytes(fmt)
        self._chk(self.L.p25fe_shard_pass1(self.h, C.c_void_p(ptr), fmt, stride, n_hist, n, abs0,
                                           C.c_void_p(result.data_ptr()), self._stream()))
        return result

    def shard_pass1_main(self, iq, offset, n_hist, abs0):
        """K1 over everything that does not need the left halo (may run while the halo is still on the wire)."""
        fmt, n_total, stride = self._iq_view(iq)
        ptr = iq.data_ptr() + offset * fmt_bytes(fmt)
        self._chk(self.L.p25fe_shard_pass1_main(self.h, C.c_void_p(ptr), fmt, stride, n_hist, n_total - offset, abs0,
                                                self._stream()))

    def shard_pass1_finish(self, iq, offset, n_hist, abs0, result=None):
        """The shard's head (needs the halo) + sync detection + scan; same arguments as shard_pass1_main."""
        import torch
        fmt, n_total, stride = self._iq_view(iq)
        if result is None:
            result = torch.empty((self.C, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=iq.device)
        ptr = iq.data_ptr() + offset * fmt_bytes(fmt)
        self._chk(self.L.p25fe_shard_pass1_finish(self.h, C.c_void_p(ptr), fmt, stride, n_hist, n_total - offset, abs0,
                                                  C.c_void_p(result.data_ptr()), self._stream()))
        return result

    def shard_pass1_head(self, iq, offset, n_hist, abs0):
        """The shard's head segment alone (needs the halo); may run on another stream beside shard_pass1_main's launch."""
        fmt, n_total, stride = self._iq_view(iq)
        ptr = iq.data_ptr() + offset * fmt_bytes(fmt)
        self._chk(self.L.p25fe_shard_pass1_head(self.h, C.c_void_p(ptr), fmt, stride, n_hist, n_total - offset, abs0,
                                                self._stream()))

    def shard_head_check(self):
        """after a synchronise: raises P25feError(ERR_TIMEOUT) if a detection gave up waiting for a head segment (p25fe_shard_head_check)"""
        self._chk(self.L.p25fe_shard_head_check(self.h))

    def shard_pipe_begin(self):
        """p25fe_shard_pipe_begin on torch's current stream -> the handle's receive stream as a torch stream: shard_pass1_main stays
        on the current stream, every later pass of the step is enqueued under `with torch.cuda.stream(rx)`; then shard_pipe_end()."""
        import torch
        rx = C.c_void_p()
        self._chk(self.L.p25fe_shard_pipe_begin(self.h, self._stream(), C.byref(rx)))
        return torch.cuda.ExternalStream(rx.value)

    def shard_pipe_end(self, last=None):
        """last: the torch stream the step's final pass was enqueued on (default: the receive stream)"""
        self._chk(self.L.p25fe_shard_pipe_end(self.h, C.c_void_p(last.cuda_stream) if last is not None else None))

    def shard_pass1_k1(self, iq, offset, n_hist, abs0):
        """The whole front end of pass 1 (main + head) in one launch; shard_pass1_finish then runs detection + scan only."""
        fmt, n_total, stride = self._iq_view(iq)
        ptr = iq.data_ptr() + offset * fmt_bytes(fmt)
        self._chk(self.L.p25fe_shard_pass1_k1(self.h, C.c_void_p(ptr), fmt, stride, n_hist, n_total - offset, abs0, self._stream()))

    def streams_share_queue(self, a, b):
        """do the torch streams a and b (None: the NULL stream) sit on one hardware queue?  (p25fe_streams_share_queue; synchronises both)"""
        sh = C.c_int(0)
        pa = C.c_void_p(a.cuda_stream) if a is not None else None
        pb = C.c_void_p(b.cuda_stream) if b is not None else None
        self._chk(self.L.p25fe_streams_share_queue(self.h, pa, pb, C.byref(sh)))
        return bool(sh.value)

    def shard_pass2_dev(self, summ_all, d_bb0, d_bbn, rank, n_bb, dibits=None, dup=None, result=None):
        """Pass 2 with the combine inside it (p25fe_shard_pass2_dev): summ_all uint8 [n_shards, sizeof(result)] on the device.
        Returns (dibits, result, anchors uint8 [n_shards, sizeof(anchor)], offsets int64 [n_shards + 1])."""
        import torch
        n = summ_all.shape[0]
        dev = summ_all.device
        cap = (n_bb // 10 + 64 + 15) // 16 * 16
        dib = dibits if dibits is not None else torch.empty((1, cap), dtype=torch.uint8, device=dev)
        if result is None:
            result = torch.empty((1, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        anchors = torch.empty((n, ANCHOR_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self._chk(self.L.p25fe_shard_pass2_dev(self.h, C.c_void_p(summ_all.data_ptr()), C.c_void_p(d_bb0.data_ptr()),
                                               C.c_void_p(d_bbn.data_ptr()), n, rank, C.c_void_p(anchors.data_ptr()),
                                               C.c_void_p(offsets.data_ptr()), C.c_void_p(dib.data_ptr()), dib.stride(0),
                                               C.c_void_p(dup.data_ptr()) if dup is not None else None,
                                               C.c_void_p(result.data_ptr()), self._stream()))
        return dib, result, anchors, offsets

    def shard_compact_from_dev(self, gathered, offsets, first, out):
        """shard_compact_dev for shards first .. n - 1 only (rank 0 has sliced its own shard into `out` already)."""
        self._chk(self.L.p25fe_shard_compact_from_dev(self.h, C.c_void_p(gathered.data_ptr()), gathered.shape[1],
                                                      C.c_void_p(offsets.data_ptr()), first, gathered.shape[0],
                                                      C.c_void_p(out.data_ptr()), out.numel(), self._stream()))
        return out

    def shard_compact_dev(self, gathered, offsets, out):
        """gathered uint8 [n_shards, cap] (all-gathered shard streams), offsets int64 [n_shards + 1] -> out uint8 [total]."""
        self._chk(self.L.p25fe_shard_compact_dev(self.h, C.c_void_p(gathered.data_ptr()), gathered.shape[1],
                                                 C.c_void_p(offsets.data_ptr()), gathered.shape[0],
                                                 C.c_void_p(out.data_ptr()), out.numel(), self._stream()))
        return out

    def shard_resolve_dev(self, summ_all, d_bb0, d_bbn, anchors=None, offsets=None):
        """Device-side combine: summ_all uint8 [n_shards, sizeof(result)], d_bb0 / d_bbn int64 device tensors.
        Returns (anchors uint8 [n_shards, sizeof(anchor)], offsets int64 [n_shards + 1], last = total) without
        synchronising."""
        import torch
        n = summ_all.shape[0]
        if anchors is None:
            anchors = torch.empty((n, ANCHOR_DTYPE.itemsize), dtype=torch.uint8, device=summ_all.device)
        if offsets is None:
            offsets = torch.empty(n + 1, dtype=torch.int64, device=summ_all.device)
        self._chk(self.L.p25fe_shard_resolve_dev(self.h, C.c_void_p(summ_all.data_ptr()), C.c_void_p(d_bb0.data_ptr()),
                                                 C.c_void_p(d_bbn.data_ptr()), n, C.c_void_p(anchors.data_ptr()),
                                                 C.c_void_p(offsets.data_ptr()), self._stream()))
        return anchors, offsets

    def shard_pass2(self, anchor_in, n_bb, device, result=None, dibits=None):
        """anchor_in: NumPy structured anchor(s) (host) or a uint8 device tensor holding one p25fe_anchor_t per channel."""
        import torch
        cap = (n_bb // 10 + 64 + 15) // 16 * 16
        dib = dibits if dibits is not None else torch.empty((self.C, cap), dtype=torch.uint8, device=device)
        if result is None:
            result = torch.empty((self.C, RESULT_DTYPE.itemsize), dtype=torch.uint8, device=device)
        if isinstance(anchor_in, torch.Tensor):
            a_in = anchor_in
        else:
            a_in = torch.from_numpy(np.frombuffer(np.asarray(anchor_in, dtype=ANCHOR_DTYPE).tobytes(), dtype=np.uint8).copy()).to(device)
        self._chk(self.L.p25fe_shard_pass2(self.h, C.c_void_p(a_in.data_ptr()), C.c_void_p(dib.data_ptr()), dib.stride(0),
                                           C.c_void_p(result.data_ptr()), self._stream()))
        return dib, result

    def shard_resolve(self, summaries, bb0, bbn):
        """Host combine of per-shard summaries (np structured RESULT_DTYPE, time order) -> (anchor_in, dibit_offset)."""
        summaries = np.ascontiguousarray(summaries, dtype=RESULT_DTYPE)
        bb0 = np.ascontiguousarray(bb0, dtype=np.uint64)
        bbn = np.ascontiguousarray(bbn, dtype=np.uint64)
        n = len(summaries)
        anc = np.zeros(n, dtype=ANCHOR_DTYPE)
        off = np.zeros(n + 1, dtype=np.uint64)                   # [n] = total dibits of the capture
        self._chk(self.L.p25fe_shard_resolve(_p(summaries), _p(bb0), _p(bbn), n, self.symbol_clock, _p(anc), _p(off)))
        return anc, off


def parse_results(t):
    """uint8 result tensor [C, sizeof(p25fe_result_t)] -> NumPy structured array (syncs the stream)."""
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=RESULT_DTYPE).copy()


def n_baseband(abs0, n):
    return _lib.load().p25fe_n_baseband(abs0, n)


class Resampler:
    """The rational resampler of docs/SPEC.md 3.0b (p25fe_resampler_t): any tuner sample rate -> 240 ksps by L / M with a
    caller-supplied polyphase table, taps[j * L + p] = tap j of phase p.  Made for one FrontEnd (its device, channel count
    and u8 conversion), which must outlive it."""

    @staticmethod
    def design(fs):
        """(L, M, T, taps) for a tuner rate in Hz (p25fe_resampler_design; needs no device)"""
        L_ = _lib.load()
        l, m, t = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        rc = L_.p25fe_resampler_design(int(fs), C.byref(l), C.byref(m), C.byref(t), None, 0)
        if rc != _lib.ERR_CAPACITY:
            _lib.check(L_, None, rc if rc != _lib.OK else _lib.ERR_ARG)
        taps = np.empty(l.value * t.value, dtype=np.float32)
        _lib.check(L_, None, L_.p25fe_resampler_design(int(fs), C.byref(l), C.byref(m), C.byref(t), _p(taps), taps.size))
        return l.value, m.value, t.value, taps

    def __init__(self, fe, L, M, T, taps):
        self.fe, self.lib = fe, fe.L
        self.L, self.M, self.T = int(L), int(M), int(T)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        if taps.size != self.L * self.T:
            raise _lib.P25feError(_lib.ERR_ARG, "the table holds L * T taps")
        self.rs = C.c_void_p()
        _lib.check(self.lib, fe.h, self.lib.p25fe_resampler_create(fe.h, self.L, self.M, self.T, _p(taps), C.byref(self.rs)))

    def close(self):
        if getattr(self, "rs", None):
            self.lib.p25fe_resampler_destroy(self.rs)
            self.rs = None

    __del__ = close

    def n_out(self, abs0, n):
        return int(self.lib.p25fe_n_resample(self.L, self.M, abs0, n))

    def reset(self):
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_resampler_reset(self.rs))

    def resample_dev(self, iq, n_hist=0, abs0=0, offset=0, out=None):
        """cf32, int16 or uint8 [n, 2] or [C, n, 2] on the device -> (cf32 [C, n_out (padded), 2], n_out); `offset` = index of the
        first owned sample inside `iq` (>= n_hist), abs0 its position in the stream."""
        import torch
        fmt, n_total, stride = self.fe._iq_view(iq)
        n = n_total - offset
        no = self.n_out(abs0, n)
        if out is None:
            out = torch.empty((self.fe.C, (no + 3) // 2 * 2, 2), dtype=torch.float32, device=iq.device)
        _lib.check(self.lib, self.fe.h,
                   self.lib.p25fe_resample_dev(self.rs, C.c_void_p(iq.data_ptr() + fmt_bytes(fmt) * offset), fmt, stride, n_hist, n, abs0,
                                               C.c_void_p(out.data_ptr()), out.stride(0) // 2, self.fe._stream()))
        return out, no

    def resample(self, iq, cap=None):
        """host streaming form: the next samples of the stream (complex64 [n] / [C, n], int16 or uint8 interleaved pairs [2 n] /
        [C, 2 n]) -> complex64 [n_out] / [C, n_out]; the object keeps the history and the position between calls"""
        iq = np.asarray(iq)
        if iq.dtype == np.uint8:
            fmt = FMT_U8
        elif iq.dtype == np.int16:
            fmt = FMT_S16
        else:
            fmt, iq = FMT_CF32, iq.astype(np.complex64, copy=False)
        Cn = self.fe.C
        iq = np.ascontiguousarray(iq).reshape(Cn, -1)
        n = iq.shape[1] if fmt == FMT_CF32 else iq.shape[1] // 2
        if cap is None:
            cap = n * self.L // self.M + 1
        out = np.empty((Cn, max(cap, 1)), dtype=np.complex64)
        no = C.c_size_t(0)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_resample(self.rs, _p(iq), fmt, n, _p(out), cap, C.byref(no)))
        res = out[:, :no.value]
        return res[0].copy() if Cn == 1 else res.copy()


class Tuner:
    """The tuner of docs/SPEC.md 3.0c (p25fe_tuner_t): K channels at rational frequency offsets out of ONE capture of any supported
    rate, each a 240 ksps cf32 row -- the resampler with a mixer in front.  freqs = [(num, den), ...] in cycles per input sample,
    lowest terms.  Made for one FrontEnd (its device and u8 conversion; its channel count does not matter), which must outlive it.
    Tuner.nco makes the other kind (SPEC 3.0d): channels at step / 2^32 cycles per input sample, any offset; its methods are these."""

    @staticmethod
    def freq(fs_hz, offset_hz):
        """(num, den) = offset_hz / fs_hz in lowest terms (p25fe_tuner_freq; needs no device)"""
        L_ = _lib.load()
        num, den = C.c_int32(0), C.c_int32(0)
        _lib.check(L_, None, L_.p25fe_tuner_freq(int(fs_hz), int(offset_hz), C.byref(num), C.byref(den)))
        return num.value, den.value

    @staticmethod
    def rotator(den):
        """(C, S) of a denominator, float32 [den] each (p25fe_tuner_rotator: the table's definition; needs no device)"""
        L_ = _lib.load()
        cs = np.empty(2 * max(int(den), 0), dtype=np.float32)
        _lib.check(L_, None, L_.p25fe_tuner_rotator(int(den), _p(cs), cs.size))
        return cs[:den].copy(), cs[den:].copy()

    @staticmethod
    def design(fs_hz, offsets_hz):
        """(L, M, T, taps, freqs) for a tuner rate and the channels' offsets from its centre in Hz"""
        L, M, T, taps = Resampler.design(fs_hz)
        return L, M, T, taps, [Tuner.freq(fs_hz, o) for o in offsets_hz]

    @staticmethod
    def nco_step(fs_hz, offset_hz):
        """step = offset_hz / fs_hz * 2^32 rounded, as a signed 32-bit integer (p25fe_nco_step; needs no device)"""
        L_ = _lib.load()
        step = C.c_int32(0)
        _lib.check(L_, None, L_.p25fe_nco_step(int(fs_hz), float(offset_hz), C.byref(step)))
        return step.value

    @staticmethod
    def nco_factor(step, n):
        """(c, s) of SPEC 3.0d for a step and an absolute index, as the kernel computes them (p25fe_nco_factor)"""
        L_ = _lib.load()
        cs = np.empty(2, dtype=np.float32)
        _lib.check(L_, None, L_.p25fe_nco_factor(int(step), int(n), _p(cs)))
        return cs[0], cs[1]

    @staticmethod
    def design_nco(fs_hz, offsets_hz):
        """(L, M, T, taps, steps) for a tuner rate and the channels' offsets from its centre in Hz (fractional offsets welcome)"""
        L, M, T, taps = Resampler.design(fs_hz)
        return L, M, T, taps, [Tuner.nco_step(fs_hz, o) for o in offsets_hz]

    def __init__(self, fe, L, M, T, taps, freqs=None, steps=None):
        self.fe, self.lib = fe, fe.L
        self.L, self.M, self.T = int(L), int(M), int(T)
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        if taps.size != self.L * self.T:
            raise _lib.P25feError(_lib.ERR_ARG, "the table holds L * T taps")
        if (freqs is None) == (steps is None):
            raise _lib.P25feError(_lib.ERR_ARG, "a tuner is one kind: freqs or steps")
        self.tn = C.c_void_p()
        if steps is not None:
            self.steps = [int(s) for s in steps]
            self.K = len(self.steps)
            step = np.array(self.steps, dtype=np.int64).astype(np.int32)
            _lib.check(self.lib, fe.h, self.lib.p25fe_nco_create(fe.h, self.L, self.M, self.T, _p(taps), self.K, _p(step),
                                                                       C.byref(self.tn)))
            return
        self.freqs = [(int(a), int(b)) for a, b in freqs]
        self.K = len(self.freqs)
        num = np.array([f[0] for f in self.freqs], dtype=np.int32)
        den = np.array([f[1] for f in self.freqs], dtype=np.int32)
        _lib.check(self.lib, fe.h, self.lib.p25fe_tuner_create(fe.h, self.L, self.M, self.T, _p(taps), self.K, _p(num), _p(den),
                                                               C.byref(self.tn)))

    @classmethod
    def nco(cls, fe, L, M, T, taps, steps):
        """a tuner of NCO channels (p25fe_nco_create): steps = signed 32-bit integers, step / 2^32 cycles per input sample"""
        return cls(fe, L, M, T, taps, steps=steps)

    def close(self):
        if getattr(self, "tn", None):
            self.lib.p25fe_tuner_destroy(self.tn)
            self.tn = None

    __del__ = close

    def n_out(self, abs0, n):
        return int(self.lib.p25fe_n_resample(self.L, self.M, abs0, n))

    def reset(self):
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_tuner_reset(self.tn))

    def set_step(self, k, step, abs_at):
        """NCO channel k goes on at `step` from the absolute index abs_at with no phase jump there (p25fe_afc_set_step, SPEC 3.0e);
        applies to the tune_dev calls issued after it on the current stream, and to tune"""
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_afc_set_step(self.tn, int(k), int(step), int(abs_at), self.fe._stream()))
        self.steps[int(k)] = int(step)

    def get_step(self, k):
        """(step, ph0) of NCO channel k as the launches issued from now on see them (p25fe_afc_get_step)"""
        step, ph0 = C.c_int32(0), C.c_uint32(0)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_afc_get_step(self.tn, int(k), C.byref(step), C.byref(ph0)))
        return step.value, ph0.value

    def tune_dev(self, iq, n_hist=0, abs0=0, offset=0, out=None):
        """cf32, int16 or uint8 [n, 2] on the device -> (cf32 [K, n_out (padded), 2], n_out); `offset` = index of the first owned
        sample inside `iq` (>= n_hist), abs0 its position in the stream.  The rows feed a K-channel FrontEnd's run_dev / demod_dev."""
        import torch
        assert iq.is_cuda and iq.dim() == 2 and iq.shape[1] == 2 and iq.is_contiguous()
        fmt = _torch_fmt(iq.dtype)
        n = iq.shape[0] - offset
        no = self.n_out(abs0, n)
        if out is None:
            out = torch.empty((self.K, (no + 3) // 2 * 2, 2), dtype=torch.float32, device=iq.device)
        _lib.check(self.lib, self.fe.h,
                   self.lib.p25fe_tune_dev(self.tn, C.c_void_p(iq.data_ptr() + fmt_bytes(fmt) * offset), fmt, n_hist, n, abs0,
                                           C.c_void_p(out.data_ptr()), out.stride(0) // 2, self.fe._stream()))
        return out, no

    def cuts(self, cuts):
        """the cuts of docs/SPEC.md 3.0j on this (NCO) tuner: a structured array of _lib.CUT_DTYPE, or (abs_first, n, step, ph0) tuples"""
        return Cuts(self, cuts)

    def tune(self, iq, cap=None):
        """host streaming form: the capture's next samples (complex64 [n], int16 or uint8 interleaved pairs [2 n]) -> complex64
        [K, n_out]; the object keeps the history and the position between calls"""
        iq = np.asarray(iq)
        if iq.dtype == np.uint8:
            fmt = FMT_U8
        elif iq.dtype == np.int16:
            fmt = FMT_S16
        else:
            fmt, iq = FMT_CF32, iq.astype(np.complex64, copy=False)
        iq = np.ascontiguousarray(iq).reshape(-1)
        n = iq.size if fmt == FMT_CF32 else iq.size // 2
        if cap is None:
            cap = n * self.L // self.M + 1
        out = np.empty((self.K, max(cap, 1)), dtype=np.complex64)
        no = C.c_size_t(0)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_tune(self.tn, _p(iq), fmt, n, _p(out), cap, C.byref(no)))
        return out[:, :no.value].copy()


class Cuts:
    """Cuts of one capture (docs/SPEC.md 3.0j, p25fe_cuts_t): J pieces {abs_first, n, step, ph0} tuned in ONE launch, each the slice of
    the row Tuner.tune_dev writes for an NCO channel (step, ph0) over the whole range, bit for bit.  Made on an NCO tuner (its table,
    rotator and device; its own channels are not used), which must outlive every use.  counts[j] is cut j's output count."""

    @staticmethod
    def from_keys(keys, N, hop, B, fs_hz, margin=0, range_first=0, range_n=0):
        """Scanner.keys' intervals -> cuts (structured array of _lib.CUT_DTYPE), clipped to [range_first, range_first + range_n)
        (p25fe_cuts_from_keys; needs no device)"""
        L_ = _lib.load()
        keys = np.ascontiguousarray(keys, dtype=_lib.WATERFALL_KEY_DTYPE)
        out = np.zeros(max(keys.size, 1), dtype=_lib.CUT_DTYPE)
        n = C.c_size_t(0)
        _lib.check(L_, None, L_.p25fe_cuts_from_keys(_p(keys), keys.size, int(N), int(hop), int(B), int(fs_hz), int(margin),
                                                     int(range_first), int(range_n), _p(out), out.size, C.byref(n)))
        return out[:n.value].copy()

    def __init__(self, tuner, cuts):
        self.tuner, self.fe, self.lib = tuner, tuner.fe, tuner.lib
        if not (isinstance(cuts, np.ndarray) and cuts.dtype == _lib.CUT_DTYPE):
            cuts = np.array([tuple(int(v) for v in c) for c in cuts], dtype=_lib.CUT_DTYPE)
        self.cuts = np.ascontiguousarray(cuts).reshape(-1)
        self.J = int(self.cuts.size)
        counts = np.zeros(max(self.J, 1), dtype=np.uintp)
        mx = C.c_size_t(0)
        self.ct = C.c_void_p()
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_cuts_create(tuner.tn, _p(self.cuts), self.J, _p(counts), C.byref(mx), C.byref(self.ct)))
        self.counts = [int(c) for c in counts[:self.J]]
        self.max_count = int(mx.value)

    def close(self):
        if getattr(self, "ct", None):
            self.lib.p25fe_cuts_destroy(self.ct)
            self.ct = None

    __del__ = close

    def tune_dev(self, iq, n_hist=0, abs0=0, offset=0, out=None, stride=None):
        """cf32, int16 or uint8 [n, 2] on the device -> cf32 [J, stride, 2]: row j holds counts[j] samples and, where this call makes
        the rows, zeros behind them (stride: even, at least max_count, max_count rounded up by default; rows 16-byte aligned), so the
        rows feed a J-channel FrontEnd's run_dev as they are.  A given `out` is written in [0, counts[j]) of each row only."""
        import torch
        assert iq.is_cuda and iq.dim() == 2 and iq.shape[1] == 2 and iq.is_contiguous()
        fmt = _torch_fmt(iq.dtype)
        n = iq.shape[0] - offset
        if out is None:
            if stride is None:
                stride = (self.max_count + 3) // 2 * 2
            assert stride % 2 == 0
            out = torch.zeros((self.J, stride, 2), dtype=torch.float32, device=iq.device)
        _lib.check(self.lib, self.fe.h,
                   self.lib.p25fe_cuts_dev(self.ct, C.c_void_p(iq.data_ptr() + fmt_bytes(fmt) * offset), fmt, n_hist, n, abs0,
                                                C.c_void_p(out.data_ptr()), out.stride(0) // 2, self.fe._stream()))
        return out


class Afc:
    """The frequency measure of docs/SPEC.md 3.0f (p25fe_afc_t): per row of 240 ksps cf32 -- a tuner's output rows -- the integer sums
    of w[m] conj(w[m-1]) and |w[m]|^2, w = the row through a real low-pass (taps, T of them) decimated by D.  Made for one FrontEnd
    (its device), which must outlive it; K rows."""

    DEFAULT = (10, 240, 7000.0)                                      # D, T, cutoff in Hz: the recommended prefilter

    @staticmethod
    def design(D=10, T=240, cutoff_hz=7000.0):
        """the prefilter's taps, float32 [T] (p25fe_afc_design; needs no device)"""
        L_ = _lib.load()
        taps = np.empty(max(int(T), 0), dtype=np.float32)
        _lib.check(L_, None, L_.p25fe_afc_design(int(D), float(cutoff_hz), int(T), _p(taps), taps.size))
        return taps

    @staticmethod
    def factor(step, ph0, n):
        """(c, s) of SPEC 3.0e for a step, a phase offset and an absolute index (p25fe_afc_factor)"""
        L_ = _lib.load()
        cs = np.empty(2, dtype=np.float32)
        _lib.check(L_, None, L_.p25fe_afc_factor(int(step), int(ph0), int(n), _p(cs)))
        return cs[0], cs[1]

    @staticmethod
    def hz(acc, D):
        """one record (an element of an AFC_ACC_DTYPE array) -> (hz, coherence) (p25fe_afc_hz; host only)"""
        L_ = _lib.load()
        rec = np.zeros(1, dtype=_lib.AFC_ACC_DTYPE)
        rec[0] = acc
        hz, coh = C.c_double(0.0), C.c_double(0.0)
        _lib.check(L_, None, L_.p25fe_afc_hz(_p(rec), int(D), C.byref(hz), C.byref(coh)))
        return hz.value, coh.value

    def __init__(self, fe, K, D=10, T=240, taps=None, cutoff_hz=7000.0):
        self.fe, self.lib = fe, fe.L
        self.K, self.D, self.T = int(K), int(D), int(T)
        taps = Afc.design(D, T, cutoff_hz) if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
        if taps.size != self.T:
            raise _lib.P25feError(_lib.ERR_ARG, "the prefilter holds T taps")
        self.afc = C.c_void_p()
        _lib.check(self.lib, fe.h, self.lib.p25fe_afc_create(fe.h, self.D, self.T, _p(taps), self.K, C.byref(self.afc)))

    def close(self):
        if getattr(self, "afc", None):
            self.lib.p25fe_afc_destroy(self.afc)
            self.afc = None

    __del__ = close

    def new_acc(self):
        """K zeroed records on the device (uint8 [K, 32]): an open window"""
        import torch
        return torch.zeros((self.K, 32), dtype=torch.uint8, device="cuda:%d" % self.fe.device)

    def measure(self, rows, n_hist=0, abs0=0, offset=0, n=None, shift=24, acc=None):
        """rows: cf32 [K, cols, 2] on the device (a tuner's output); the range is samples [offset, offset + n) of every row, abs0 the
        position of its first sample, n_hist valid samples before it.  ADDS into acc (new_acc() when None) and returns it."""
        assert rows.is_cuda and rows.dim() == 3 and rows.shape[0] == self.K and rows.shape[2] == 2 and rows.stride(2) == 1
        assert rows.stride(1) == 2 and rows.stride(0) % 2 == 0
        if n is None:
            n = rows.shape[1] - offset
        assert 0 <= n_hist <= offset and offset + n <= rows.shape[1]
        if acc is None:
            acc = self.new_acc()
        _lib.check(self.lib, self.fe.h,
                   self.lib.p25fe_afc_measure_dev(self.afc, C.c_void_p(rows.data_ptr() + 8 * offset), rows.stride(0) // 2, n_hist, n, abs0,
                                                  int(shift), C.c_void_p(acc.data_ptr()), self.fe._stream()))
        return acc

    @staticmethod
    def records(acc):
        """the device records -> NumPy structured array [K] (syncs the stream)"""
        return np.frombuffer(acc.cpu().numpy().tobytes(), dtype=_lib.AFC_ACC_DTYPE).copy()


class AfcLoop:
    """The AFC loop of docs/SPEC.md 3.0g (p25fe_track_t): every channel's (step, ph0) of an NCO Tuner updated on the device from the
    records of an Afc's measure, in stream order -- tune -> measure -> update -> tune with no record read by the host.  cfg: shift,
    min_products, coh_min_q15, gain_q16, max_pull, max_dev (p25fe_track_cfg_t).  The tuner and the measure must outlive it.  After
    update / tune_tracked_dev the tuner's set_step / get_step refuse until read()."""

    DEFAULT = dict(shift=24, min_products=600, coh_min_q15=24576, gain_q16=65536, max_pull=1 << 24, max_dev=1 << 24)
    STATUS = {_lib.TRACK_NONE: "none", _lib.TRACK_SHORT: "short", _lib.TRACK_REJECT: "reject", _lib.TRACK_APPLY: "apply"}

    @staticmethod
    def config(**cfg):
        """a p25fe_track_cfg_t (TRACK_CFG_DTYPE [1]) from DEFAULT and the overrides"""
        c = np.zeros(1, dtype=_lib.TRACK_CFG_DTYPE)
        for k, v in dict(AfcLoop.DEFAULT, **cfg).items():
            c[k] = v
        return c

    @staticmethod
    def step(cfg, L, M, D, step_ref, acc, state, abs_at):
        """one channel's update on the host with the kernel's operations (p25fe_track_step): (acc', state')"""
        L_ = _lib.load()
        c = cfg if isinstance(cfg, np.ndarray) else AfcLoop.config(**cfg)
        a, s = np.zeros(1, dtype=_lib.AFC_ACC_DTYPE), np.zeros(1, dtype=_lib.TRACK_STATE_DTYPE)
        a[0] = tuple(acc)
        s[0] = tuple(state[f] for f in _lib.TRACK_STATE_DTYPE.names) if isinstance(state, dict) else tuple(state)
        _lib.check(L_, None, L_.p25fe_track_step(_p(c), int(L), int(M), int(D), int(step_ref), _p(a), _p(s), int(abs_at), _p(a), _p(s)))
        return a[0].copy(), s[0].copy()

    @staticmethod
    def hz(state, D):
        """last_theta of a state record in Hz (p25fe_track_hz)"""
        L_ = _lib.load()
        s = np.zeros(1, dtype=_lib.TRACK_STATE_DTYPE)
        s[0] = tuple(state[f] for f in _lib.TRACK_STATE_DTYPE.names) if isinstance(state, dict) else tuple(state)
        hz = C.c_double(0.0)
        _lib.check(L_, None, L_.p25fe_track_hz(_p(s), int(D), C.byref(hz)))
        return hz.value

    def __init__(self, tuner, afc, **cfg):
        self.tuner, self.afc, self.fe, self.lib = tuner, afc, tuner.fe, tuner.fe.L
        self.K = tuner.K
        self.cfg = AfcLoop.config(**cfg)
        self.lp = C.c_void_p()
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_track_create(tuner.tn, afc.afc, _p(self.cfg), C.byref(self.lp)))

    def close(self):
        if getattr(self, "lp", None):
            self.lib.p25fe_track_destroy(self.lp)
            self.lp = None

    __del__ = close

    def measure(self, rows, n_hist=0, abs0=0, offset=0, n=None):
        """Afc.measure into the loop's own records with the configuration's shift"""
        assert rows.is_cuda and rows.dim() == 3 and rows.shape[0] == self.K and rows.shape[2] == 2 and rows.stride(2) == 1
        assert rows.stride(1) == 2 and rows.stride(0) % 2 == 0
        if n is None:
            n = rows.shape[1] - offset
        assert 0 <= n_hist <= offset and offset + n <= rows.shape[1]
        _lib.check(self.lib, self.fe.h,
                   self.lib.p25fe_track_measure_dev(self.lp, C.c_void_p(rows.data_ptr() + 8 * offset), rows.stride(0) // 2, n_hist, n, abs0,
                                                    self.fe._stream()))

    def records(self, set=None):
        """the K open records (AFC_ACC_DTYPE [K]), then overwritten from `set` when given (p25fe_track_records; synchronous)"""
        got = np.zeros(self.K, dtype=_lib.AFC_ACC_DTYPE)
        new = None
        if set is not None:
            new = np.ascontiguousarray(set, dtype=_lib.AFC_ACC_DTYPE)
            assert new.shape == (self.K,)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_track_records(self.lp, _p(got), None if new is None else _p(new)))
        return got

    def update(self, abs_at):
        """every channel's update at the absolute input index abs_at: one launch on the current stream, nothing synchronised"""
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_track_update_dev(self.lp, int(abs_at), self.fe._stream()))

    def tune_tracked_dev(self, iq, window, n_hist=0, abs0=0, offset=0, out=None, out_offset=0, n_hist_out=0):
        """Tuner.tune_dev with the loop closed (p25fe_track_run_dev): the range is cut at the absolute multiples of `window` input
        samples, each piece tuned and measured, every boundary reached updated.  out (cf32 [K, cols, 2]) receives the rows from
        column out_offset on, n_hist_out valid columns before it.  -> (out, n_out)"""
        import torch
        assert iq.is_cuda and iq.dim() == 2 and iq.shape[1] == 2 and iq.is_contiguous()
        fmt = _torch_fmt(iq.dtype)
        n = iq.shape[0] - offset
        no = self.tuner.n_out(abs0, n)
        if out is None:
            out = torch.empty((self.K, out_offset + (no + 3) // 2 * 2, 2), dtype=torch.float32, device=iq.device)
        assert n_hist_out <= out_offset and out_offset + no <= out.shape[1]
        _lib.check(self.lib, self.fe.h,
                   self.lib.p25fe_track_run_dev(self.lp, C.c_void_p(iq.data_ptr() + fmt_bytes(fmt) * offset), fmt, n_hist, n, abs0,
                                                int(window), C.c_void_p(out.data_ptr() + 8 * out_offset), out.stride(0) // 2,
                                                n_hist_out, self.fe._stream()))
        return out, no

    def read(self):
        """the K state records (TRACK_STATE_DTYPE [K]); synchronous; the tuner's host pair is fresh again afterwards"""
        st = np.zeros(self.K, dtype=_lib.TRACK_STATE_DTYPE)
        _lib.check(self.lib, self.fe.h, self.lib.p25fe_track_read(self.lp, _p(st)))
        self.tuner.steps = [int(s) for s in st["step"]]
        return st
