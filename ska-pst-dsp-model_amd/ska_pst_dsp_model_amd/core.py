"""Plans and the Matlab-shaped functional API of the PFB hot path.

    polyphase_analysis(in, filt, block, os_factor)          polyphase_analysis.m:1-7
    polyphase_analysis_padded(in, filt, block, os_factor)   polyphase_analysis_padded.m:1-7
    polyphase_synthesis(in, spans_nyq, Nf, os, deripple,
                        sample_offset, overlap, t_taper,
                        s_taper, combine)                    polyphase_synthesis.m:1-13

Arrays follow the Matlab shapes: analysis input (n_pol, 1, n_dat), channelised data
(n_pol, n_chan, n_dat), synthesis output (n_pol, 1, n_out).  Channelised arrays are
returned as a transposed *view* of a (n_pol, n_dat, n_chan) buffer — the per-pol
Matlab memory order (channel fastest), which is what the kernels read and write.

Inputs may be NumPy arrays (host; the C ABI stages them through device buffers) or
``torch`` tensors on a ROCm device (zero copy on the current stream).  Every call
goes through the HIP kernels of ``libpfb_hip.so``; there is no CPU fallback.
"""
from __future__ import annotations

import hashlib
from ctypes import byref, c_double, c_int64, c_void_p

import numpy as np

from . import _lib
from .config import as_rational
from .window import PFBWindow, Taper, identity_taper

__all__ = ["AnalysisPlan", "SynthesisPlan", "polyphase_analysis", "polyphase_analysis_padded",
           "polyphase_analysis_lowcbf",
           "polyphase_synthesis", "analysis_plan", "synthesis_plan", "is_device_array",
           "roundtrip", "calc_output_nbins"]


def _torch():
    try:
        import torch  # noqa: F401
        return torch
    except Exception:  # pragma: no cover - torch is plumbing only
        return None


def is_device_array(x) -> bool:
    t = _torch()
    return t is not None and isinstance(x, t.Tensor) and x.is_cuda


def _stream_of(x, *plans):
    """The current stream of ``x``'s device as a C handle.  ``plans`` launched on it are
    marked when the stream is being captured into a graph (``close`` then refuses)."""
    t = _torch()
    s = t.cuda.current_stream(x.device)
    if plans and t.cuda.is_current_stream_capturing():
        for p in plans:
            p._capture_streams.append(s)
    return c_void_p(s.cuda_stream)


def _capturing(plan) -> bool:
    """Is a stream capture that recorded launches of ``plan`` still active?"""
    t = _torch()
    live = []
    for s in plan._capture_streams:
        with t.cuda.stream(s):
            if t.cuda.is_current_stream_capturing():
                live.append(s)
    plan._capture_streams = live
    return bool(live)


def _keep_alive(plan, tensor, device):
    """Keep ``tensor`` alive for the launches just enqueued on ``device``'s current stream,
    which read it (it may be a temporary: a ``.contiguous()`` or ``_prep_in`` copy).  Outside a
    capture its memory may be reused only after that work has finished (``record_stream``).
    A captured launch holds the address for every replay: the plan then keeps the tensor as
    long as it lives (one entry per address, so recaptures do not grow it)."""
    t = _torch()
    if t.cuda.is_current_stream_capturing():
        plan._graph_inputs[tensor.data_ptr()] = tensor
    else:
        tensor.record_stream(t.cuda.current_stream(device))


def _taps64(filt) -> np.ndarray:
    if is_device_array(filt):
        filt = filt.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(filt, dtype=np.float64).ravel())


# ============================================================================ sizes and names
_SECTION_TYPES = {8: "int8", 16: "int16", 32: "float32", 64: "float64"}


def _section_samples(raw, values: int, nbit: int, ndim: int, lowcbf: bool) -> int:
    """Time samples the section tensor ``raw`` holds, at ``values`` numbers of ``ndim``
    components of ``nbit`` bits per sample (n_pol for a single-channel section, n_chan * n_pol
    for a channelised one), as ``layout.dada_unpack`` infers them: whole samples, and whole
    heaps of 32 of a LowCBF section.  0 for a format the C ABI rejects."""
    if int(nbit) not in _SECTION_TYPES or int(ndim) not in (1, 2):
        return 0
    n_dat = (raw.numel() * raw.element_size()) // (values * int(ndim) * (int(nbit) // 8))
    return n_dat - n_dat % 32 if lowcbf else n_dat


def _section(raw, who: str, values: int, nbit: int, ndim: int, lowcbf: bool):
    """-> (the section, contiguous; its ``_section_samples``).  The DADA entries are
    device-only: a host array is answered as the C ABI would."""
    if not is_device_array(raw):
        raise _lib.PfbError(_lib.PFB_ERR_INVALID_ARG, f"{who}: expects a device tensor")
    raw = raw.contiguous()
    return raw, _section_samples(raw, values, nbit, ndim, lowcbf)


def _alloc_section(shape, nbit: int, device):
    """-> (device tensor of the DADA sample type, its bytes); a format the C ABI rejects gets
    an empty byte tensor to stand in."""
    t = _torch()
    if int(nbit) not in _SECTION_TYPES:
        return t.empty((0,) + tuple(shape[1:]), dtype=t.int8, device=device), 0
    sec = t.empty(tuple(max(int(v), 0) for v in shape), dtype=getattr(t, _SECTION_TYPES[int(nbit)]),
                  device=device)
    return sec, sec.numel() * sec.element_size()


def _order(lowcbf: bool) -> int:
    return _lib.PFB_DADA_LOWCBF if lowcbf else _lib.PFB_DADA_TFP


# what the plans' last_* getters report (anything else, 0 and -1 included: 'none')
_DADA_INPUT_NAMES = {_lib.PFB_DADA_INPUT_FUSED: "fused", _lib.PFB_DADA_INPUT_STAGED: "staged"}
_DADA_OUTPUT_NAMES = {_lib.PFB_DADA_OUTPUT_FUSED: "fused", _lib.PFB_DADA_OUTPUT_STAGED: "staged"}
_QUANTISER_NAMES = {_lib.PFB_QUANTISER_FUSED: "fused", _lib.PFB_QUANTISER_STAGED: "staged"}
_INPUT_QUANTISER_NAMES = {_lib.PFB_INPUT_QUANTISER_FUSED: "fused", _lib.PFB_INPUT_QUANTISER_STAGED: "staged"}
_STRIDED_INPUT_NAMES = {_lib.PFB_STRIDED_INPUT_IN_PLACE: "in_place",
                        _lib.PFB_STRIDED_INPUT_STAGED: "staged"}
_STAGE1_NAMES = {_lib.PFB_STAGE1_STORED: "stored", _lib.PFB_STAGE1_RECOMPUTED: "recomputed"}


def _mode_name(plan, getter: str, names: dict) -> str:
    return names.get(int(getattr(plan._lib, getter)(plan._h)), "none")


class _Plan:
    """What the two plan classes share: the C handle and its lifetime."""

    _destroy = None  # the subclass's pfb_*_plan_destroy

    def __init__(self):
        # first, before anything can raise: a constructor that fails leaves an object whose
        # __del__ finds every attribute close() reads
        self._h = None
        self._capture_streams = []  # streams that captured launches of this plan
        self._rt_input = None       # the input of a split round trip in flight (roundtrip_analysis)
        self._graph_inputs = {}     # tensors that captured launches read, by address (_keep_alive)
        self._lib = _lib.load()
        _lib.require_device()

    def close(self):
        if self._h:
            # A captured graph references the plan's device buffers (taps, twiddles, stage-1
            # rows, carry) by address: freeing them while the capture is open, or before every
            # graph that replays them is gone, makes the replays read freed memory
            # (INTEGRATION.md §3).
            if self._capture_streams and _capturing(self):
                raise RuntimeError(f"{type(self).__name__}.close(): a stream capture that used this "
                                   "plan is still active; end the capture (and drop its graphs) first")
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ============================================================================ analysis
class AnalysisPlan(_Plan):
    """Device plan of one analysis filter bank (owns taps, twiddles, carry-over)."""

    _destroy = "pfb_analysis_plan_destroy"

    def __init__(self, taps, n_chan: int, os_factor, variant: str = "polyphase_analysis",
                 n_pol: int = 1, device: int = 0):
        super().__init__()
        self.os_factor = as_rational(os_factor)
        self.n_chan = int(n_chan)
        self.n_pol = int(n_pol)
        self.device = int(device)
        self.variant = variant
        v = {"polyphase_analysis": _lib.PFB_ANALYSIS_BUNTON, "bunton": _lib.PFB_ANALYSIS_BUNTON,
             "polyphase_analysis_padded": _lib.PFB_ANALYSIS_PADDED,
             "padded": _lib.PFB_ANALYSIS_PADDED,
             "polyphase_analysis_lowcbf": _lib.PFB_ANALYSIS_LOWCBF,
             "lowcbf": _lib.PFB_ANALYSIS_LOWCBF}
        if variant not in v:
            raise ValueError(f"unknown analysis function '{variant}'")
        self.taps = _taps64(taps)
        arr, ptr = _lib.c_double_array(self.taps)
        d = _lib.AnalysisDesc(v[variant], self.n_chan, self.os_factor.nu, self.os_factor.de,
                              ptr, len(arr), self.n_pol, self.device)
        h = c_void_p()
        _lib.check(self._lib.pfb_analysis_plan_create(byref(d), byref(h)))
        self._h = h
        self.out_chan = int(self._lib.pfb_analysis_output_channels(h))  # 216 for LowCBF
        self.step = (self.n_chan * self.os_factor.de) // self.os_factor.nu
        self.phases = -(-len(self.taps) // self.n_chan)

    def output_length(self, n_dat: int) -> int:
        return int(self._lib.pfb_analysis_output_length(self._h, int(n_dat)))

    @property
    def buffered_samples(self) -> int:
        return int(self._lib.pfb_filterbank_buffered(self._h))

    def reset(self):
        _lib.check(self._lib.pfb_filterbank_reset(self._h))

    def stream_rows(self, n_in: int) -> int:
        """Rows the next stateful execute of n_in samples returns (nu-trimmed)."""
        return int(self._lib.pfb_filterbank_output_rows(self._h, int(n_in)))

    def execute_strided(self, x, out, out_pol_stride: int, row_stride: int, chan_stride: int,
                        sel=(0, 0, 0)):
        """Stateful execute of device series ``x`` (n_pol, n_dat; any pol stride, unit
        sample stride) writing bin c of row k of pol p to
        ``out``'s storage at p * out_pol_stride + k * row_stride + j * chan_stride
        (``pfb_filterbank_execute_strided``; sel = (split, shift, n) is the cascade's
        channel chomp).  Returns the number of rows written.  Plans: ``polyphase_analysis``
        on the streaming kernel (N = 256) and every ``polyphase_analysis_padded`` plan;
        others raise ``PfbError`` with ``PFB_ERR_UNSUPPORTED``.  A padded plan stores exactly
        the returned T_out rows: the rows [T_out, K) of its circular shift are dropped at
        the store (no scratch rows in ``out``, no staging copy), with guarded plain stores,
        so the layout's extent is limited only by ``out``'s capacity."""
        if x.shape[0] != self.n_pol or x.stride(1) != 1:
            raise ValueError("execute_strided: (n_pol, n_dat) series with unit sample stride")
        n_dat = int(x.shape[1])
        # elements of out's storage from its first element (the C ABI range-checks the
        # furthest strided write against it)
        cap = out.untyped_storage().nbytes() // out.element_size() - out.storage_offset()
        n_out = c_int64(0)
        # (a single series' stride(0) is arbitrary in torch; the C ABI checks the pol stride
        # against n_dat whatever n_pol is)
        in_ps = x.stride(0) if x.shape[0] > 1 else n_dat
        _lib.check(self._lib.pfb_filterbank_execute_strided(
            self._h, c_void_p(x.data_ptr()), in_ps, n_dat, c_void_p(out.data_ptr()),
            int(out_pol_stride), int(row_stride), int(chan_stride), int(sel[0]), int(sel[1]),
            int(sel[2]), int(cap), byref(n_out), _stream_of(x, self)))
        return int(n_out.value)

    def _prep_in(self, x):
        """-> (array (n_pol, n_dat) complex64 contiguous, is_device)."""
        if is_device_array(x):
            t = _torch()
            x = x.to(t.complex64)
            if x.dim() == 3:
                x = x[:, 0, :]
            elif x.dim() == 1:
                x = x[None, :]
            x = x.contiguous()
            return x, True
        x = np.asarray(x)
        if x.ndim == 3:
            x = x[:, 0, :]
        elif x.ndim == 1:
            x = x[None, :]
        x = np.ascontiguousarray(x, dtype=np.complex64)
        return x, False

    def _alloc_out(self, like, dev, rows):
        if dev:
            t = _torch()
            return t.empty((self.n_pol, max(rows, 0), self.out_chan), dtype=t.complex64,
                           device=like.device)
        return np.empty((self.n_pol, max(rows, 0), self.out_chan), dtype=np.complex64)

    # Two row-capacity rules, different on purpose (keep both):
    #
    # _buffer_rows, the cf32 calls.  A stateful call returns Kt = K - K % nu rows of the K the
    # buffered and new samples make, but a padded plan COMPUTES all K: its circular shift runs
    # over every row (filterbank_exec: Krun = K).  The launch stores straight into the caller's
    # buffer only when that has room for all Krun rows, rows [Kt, K) being scratch; otherwise it
    # goes through the plan's staging buffer and a copy of Kt rows (fb_rows_dst).  K is at most
    # (buffered + n) // step (the padded plan's own count; the others' is smaller), so one row
    # more than that always has the room.
    #
    # _section_rows, the to-DADA calls.  The section gets exactly the Kt rows returned
    # (pfb_filterbank_output_rows = fb_lens().Kt) and never scratch rows: analysis_to_dada has
    # the store kernel write rows below Kt only, or runs the cf32 path into the plan's own K-row
    # buffer and packs Kt rows from it, and checks the section's bytes against Kt rows alone.
    # (pfb_filterbank_execute_strided drops rows [Kt, K) at the store in the same way.)
    def _buffer_rows(self, n_dat: int, stateful: bool) -> int:
        if stateful:
            return (self.buffered_samples + n_dat) // max(self.step, 1) + 1
        return self.output_length(n_dat)

    def _section_rows(self, n_dat: int, stateful: bool) -> int:
        return self.stream_rows(n_dat) if stateful else self.output_length(n_dat)

    def execute(self, x, stateful: bool = False):
        """Run the analysis; returns the (n_pol, K, n_chan) buffer (time-major)."""
        x, dev = self._prep_in(x)
        if x.shape[0] != self.n_pol:
            raise ValueError(f"plan built for n_pol={self.n_pol}, got {x.shape[0]}")
        n_dat = x.shape[1]
        cap = self._buffer_rows(n_dat, stateful)
        out = self._alloc_out(x, dev, cap)
        n_out = c_int64(0)
        if dev:
            src, dst, mem, stream = c_void_p(x.data_ptr()), c_void_p(out.data_ptr()), \
                _lib.PFB_MEM_DEVICE, _stream_of(x, self)
        else:
            src, dst, mem, stream = x.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p), \
                _lib.PFB_MEM_HOST, c_void_p(0)
        fn = self._lib.pfb_filterbank_execute if stateful else self._lib.pfb_analysis_execute
        _lib.check(fn(self._h, src, n_dat, n_dat, dst, cap * self.out_chan, cap, byref(n_out),
                      mem, stream))
        return out[:, :n_out.value, :]

    def execute_dada(self, raw, nbit: int, ndim: int = 2, lowcbf: bool = False, stateful: bool = False):
        """The analysis of a single-channel DADA data section (``raw``: a device tensor of
        bytes or samples, n_dat x n_pol x ndim values of nbit in TFP or LowCBF order, the
        polarisations interleaved as the file holds them) — bit for bit
        ``execute(layout.dada_unpack(raw, nbit, ndim, 1, n_pol)[:, :, 0])``, without the
        unpacked series crossing HBM where the analysis kernel can load the section itself
        (pfb_analysis_execute_dada / pfb_filterbank_execute_dada; ``last_dada_input()``
        tells).  n_dat is inferred as ``layout.dada_unpack`` does.  Returns the
        (n_pol, K, n_chan) buffer like ``execute``."""
        raw, n_dat = _section(raw, "execute_dada", self.n_pol, nbit, ndim, lowcbf)
        cap = self._buffer_rows(n_dat, stateful)
        out = self._alloc_out(raw, True, cap)
        n_out = c_int64(0)
        fn = self._lib.pfb_filterbank_execute_dada if stateful else self._lib.pfb_analysis_execute_dada
        _lib.check(fn(self._h, c_void_p(raw.data_ptr()), int(nbit), int(ndim), _order(lowcbf), n_dat,
                      c_void_p(out.data_ptr()), cap * self.out_chan, cap, byref(n_out), _stream_of(raw, self)))
        return out[:, :n_out.value, :]

    def last_dada_input(self) -> str:
        """How the plan's last DADA call read its section: 'fused' (the analysis kernel
        loaded the file's own bytes), 'staged' (unpacked first), 'none' (no DADA call, or a
        cf32 call since) — pfb_analysis_last_dada_input."""
        return _mode_name(self, "pfb_analysis_last_dada_input", _DADA_INPUT_NAMES)

    def execute_to_dada(self, x, out_nbit: int, scale: float = 1.0, stateful: bool = False):
        """The analysis of device series ``x`` written as a DADA data section: bit for bit
        ``layout.dada_pack(float32(scale) * execute(x), out_nbit)`` — TFP order, NDIM 2 —
        without the complex float32 product crossing HBM where the analysis kernel can store
        the samples itself (pfb_analysis_execute_to_dada / pfb_filterbank_execute_to_dada;
        ``last_dada_output()`` tells).  Returns a device tensor of shape
        (K, n_chan, n_pol, 2), int8 / int16 / float32 / float64."""
        if not is_device_array(x):
            raise _lib.PfbError(_lib.PFB_ERR_INVALID_ARG, "execute_to_dada: expects a device tensor")
        x, _ = self._prep_in(x)
        if x.shape[0] != self.n_pol:
            raise ValueError(f"plan built for n_pol={self.n_pol}, got {x.shape[0]}")
        n_dat = x.shape[1]
        sec, nbytes = _alloc_section((self._section_rows(n_dat, stateful), self.out_chan, self.n_pol, 2),
                                     out_nbit, x.device)
        n_out = c_int64(0)
        fn = self._lib.pfb_filterbank_execute_to_dada if stateful else self._lib.pfb_analysis_execute_to_dada
        _lib.check(fn(self._h, c_void_p(x.data_ptr()), n_dat, n_dat, c_void_p(sec.data_ptr()), int(out_nbit),
                      float(scale), nbytes, byref(n_out), _stream_of(x, self)))
        return sec[:n_out.value]

    def execute_dada_to_dada(self, raw, nbit: int, out_nbit: int, scale: float = 1.0, ndim: int = 2,
                             lowcbf: bool = False, stateful: bool = False):
        """``execute_dada`` written as a DADA data section like ``execute_to_dada``: file
        bytes in, file bytes out (pfb_analysis_execute_dada_to_dada /
        pfb_filterbank_execute_dada_to_dada); ``last_dada_input()`` and
        ``last_dada_output()`` tell which sides the kernel read and wrote in place."""
        raw, n_dat = _section(raw, "execute_dada_to_dada", self.n_pol, nbit, ndim, lowcbf)
        sec, nbytes = _alloc_section((self._section_rows(n_dat, stateful), self.out_chan, self.n_pol, 2),
                                     out_nbit, raw.device)
        n_out = c_int64(0)
        fn = self._lib.pfb_filterbank_execute_dada_to_dada if stateful else \
            self._lib.pfb_analysis_execute_dada_to_dada
        _lib.check(fn(self._h, c_void_p(raw.data_ptr()), int(nbit), int(ndim), _order(lowcbf), n_dat,
                      c_void_p(sec.data_ptr()), int(out_nbit), float(scale), nbytes, byref(n_out),
                      _stream_of(raw, self)))
        return sec[:n_out.value]

    def last_dada_output(self) -> str:
        """How the plan's last to-DADA call wrote its section: 'fused' (the analysis kernel
        stored the file's own bytes), 'staged' (the cf32 product packed by a second launch),
        'none' (no such call, or a cf32-output call since) — pfb_analysis_last_dada_output."""
        return _mode_name(self, "pfb_analysis_last_dada_output", _DADA_OUTPUT_NAMES)

    def _quantised(self, fn, src, head: tuple, n_dat: int, out_nbit: int, rms: float, scale: float,
                   stateful: bool, return_scale: bool):
        """The shared tail of the quantised to-DADA calls: the section of ``_section_rows``
        rows, the call, and the quantiser's scale when asked for (the call then waits)."""
        sec, nbytes = _alloc_section((self._section_rows(n_dat, stateful), self.out_chan, self.n_pol, 2),
                                     out_nbit, src.device)
        n_out = c_int64(0)
        got = c_double(1.0)
        _lib.check(fn(self._h, c_void_p(src.data_ptr()), *head, n_dat, float(rms), c_void_p(sec.data_ptr()),
                      int(out_nbit), float(scale), nbytes, byref(n_out),
                      byref(got) if return_scale else None, _stream_of(src, self)))
        _keep_alive(self, src, src.device)
        sec = sec[:n_out.value]
        return (sec, float(got.value)) if return_scale else sec

    def execute_quantised_to_dada(self, x, nbit: int, rms: float, scale: float = 1.0, stateful: bool = False,
                                  return_scale: bool = False):
        """The FilterBank's rms-scaled, rounded product written as a DADA data section
        (FilterBank.m:106-113, then the file's cast): with ``y = execute(x)`` and
        ``s = rms / std(y)`` (1 when ``rms <= 0``), bit for bit
        ``layout.dada_pack(float32(scale) * round(float32(s) * y), nbit)`` — the moments summed by
        the analysis kernel and one pass over the product where the plan is on the streaming
        kernel (pfb_analysis_execute_quantised_to_dada / pfb_filterbank_execute_quantised_to_dada;
        ``last_quantiser()`` tells).  Shapes and dtypes as ``execute_to_dada``; with
        ``return_scale`` -> (section, s), and the call waits for the device."""
        if not is_device_array(x):
            raise _lib.PfbError(_lib.PFB_ERR_INVALID_ARG, "execute_quantised_to_dada: expects a device tensor")
        x, _ = self._prep_in(x)
        if x.shape[0] != self.n_pol:
            raise ValueError(f"plan built for n_pol={self.n_pol}, got {x.shape[0]}")
        n_dat = x.shape[1]
        fn = self._lib.pfb_filterbank_execute_quantised_to_dada if stateful else \
            self._lib.pfb_analysis_execute_quantised_to_dada
        return self._quantised(fn, x, (n_dat,), n_dat, nbit, rms, scale, stateful, return_scale)

    def execute_dada_quantised_to_dada(self, raw, in_nbit: int, out_nbit: int, rms: float, scale: float = 1.0,
                                       ndim: int = 2, lowcbf: bool = False, stateful: bool = False,
                                       return_scale: bool = False):
        """``execute_quantised_to_dada`` of a single-channel DADA data section, read as
        ``execute_dada`` reads it (pfb_analysis_execute_dada_quantised_to_dada /
        pfb_filterbank_execute_dada_quantised_to_dada)."""
        raw, n_dat = _section(raw, "execute_dada_quantised_to_dada", self.n_pol, in_nbit, ndim, lowcbf)
        fn = self._lib.pfb_filterbank_execute_dada_quantised_to_dada if stateful else \
            self._lib.pfb_analysis_execute_dada_quantised_to_dada
        return self._quantised(fn, raw, (int(in_nbit), int(ndim), _order(lowcbf)), n_dat, out_nbit, rms, scale,
                               stateful, return_scale)

    def set_quantiser_moments(self, mode: str):
        """Where the quantised calls take the product's moments: 'auto' (in the analysis kernel
        where the plan is on the streaming kernel), 'fused' (there or PFB_ERR_UNSUPPORTED),
        'staged' (always from the stored product) — pfb_analysis_set_quantiser_moments."""
        modes = {"auto": _lib.PFB_QUANTISER_MOMENTS_AUTO, "fused": _lib.PFB_QUANTISER_MOMENTS_FUSED,
                 "staged": _lib.PFB_QUANTISER_MOMENTS_STAGED}
        if mode not in modes:
            raise ValueError(f"quantiser moments mode {mode!r}: one of {sorted(modes)}")
        _lib.check(self._lib.pfb_analysis_set_quantiser_moments(self._h, modes[mode]))

    def last_quantiser(self) -> str:
        """The path of the plan's last quantised to-DADA call: 'fused', 'staged', or 'none' (no
        such call, or another execute call since) — pfb_analysis_last_quantiser."""
        return _mode_name(self, "pfb_analysis_last_quantiser", _QUANTISER_NAMES)

    def set_input_quantiser(self, rms):
        """The FilterBank's input quantiser (FilterBank.m:75-83) as a property of the plan: with
        ``rms`` a number, every execute call replaces its own new samples by
        ``round(float32(s) * x)``, ``s = rms / std(x)`` over the call's new samples of every
        polarisation (``rms <= 0``: round only), before the carried samples are put in front;
        ``None`` turns it off (the default) — pfb_analysis_set_input_quantiser.  Takes effect at
        the next call; may be set with samples buffered."""
        on = rms is not None
        _lib.check(self._lib.pfb_analysis_set_input_quantiser(self._h, int(on), float(rms) if on else 0.0))

    def set_input_quantiser_mode(self, mode: str):
        """Where the input quantiser rounds: 'auto' (at the analysis kernel's load where the call
        reads its new samples in place on the streaming kernel), 'fused' (there or
        PFB_ERR_UNSUPPORTED), 'staged' (always a quantising copy first) —
        pfb_analysis_set_input_quantiser_mode."""
        modes = {"auto": _lib.PFB_QUANTISER_MOMENTS_AUTO, "fused": _lib.PFB_QUANTISER_MOMENTS_FUSED,
                 "staged": _lib.PFB_QUANTISER_MOMENTS_STAGED}
        if mode not in modes:
            raise ValueError(f"input quantiser mode {mode!r}: one of {sorted(modes)}")
        _lib.check(self._lib.pfb_analysis_set_input_quantiser_mode(self._h, modes[mode]))

    def last_input_quantiser(self) -> str:
        """The input quantiser's path in the plan's last call: 'fused', 'staged', or 'none' (off,
        or no call yet) — pfb_analysis_last_input_quantiser."""
        return _mode_name(self, "pfb_analysis_last_input_quantiser", _INPUT_QUANTISER_NAMES)

    def last_input_scale(self) -> float:
        """The scale the input quantiser took in the plan's last call (1 for a round-only call or
        one without samples); waits for the device — pfb_analysis_last_input_scale."""
        t = _torch()
        got = c_double(1.0)
        stream = c_void_p(t.cuda.current_stream(t.device("cuda", self.device)).cuda_stream)
        _lib.check(self._lib.pfb_analysis_last_input_scale(self._h, byref(got), stream))
        return float(got.value)


# ============================================================================ synthesis
def _resolve_taper(taper, nf: int, ov: int, spectral_length: int = 0):
    """Translate a taper handle into (kind, coeffs) for the C ABI.  ``spectral_length``
    > 0: the handle is a SPECTRAL taper over the L = spectral_length stitched bins
    (polyphase_synthesis.m:282); custom coefficients must then number L."""
    if taper is None or taper is identity_taper:
        return _lib.PFB_WINDOW_NONE, None
    if isinstance(taper, str):
        taper = PFBWindow().lookup[taper](nf, ov)
    if isinstance(taper, Taper) and spectral_length:
        if taper.kind == _lib.PFB_WINDOW_CUSTOM:
            c = np.asarray(taper.coeffs, dtype=np.float64).ravel()
            if c.size != spectral_length:
                raise ValueError(f"custom spectral taper needs {spectral_length} coefficients, "
                                 f"got {c.size}")
            return taper.kind, c
        return taper.kind, None  # hann: the plan builds circshift(hann(L), L/2)
    if isinstance(taper, Taper):
        if taper.kind == _lib.PFB_WINDOW_CUSTOM:
            return taper.kind, np.asarray(taper.coeffs, dtype=np.float64)
        if taper.kind in (_lib.PFB_WINDOW_TUKEY, _lib.PFB_WINDOW_TOP_HAT) and \
                (taper.input_fft_length, taper.input_discard) != (nf, ov):
            # the Matlab handle closes over its own (Nf, Ov); honour them explicitly
            return _lib.PFB_WINDOW_CUSTOM, taper.time_window(nf)
        return taper.kind, None
    kind = getattr(taper, "kind", None)
    if kind == _lib.PFB_WINDOW_NONE:
        return kind, None
    raise TypeError("polyphase_synthesis: arbitrary Python taper callables cannot run on the "
                    "GPU path; use a PFBWindow taper or PFBWindow().custom(coeffs)")


def _resolve_deripple(deripple):
    if deripple is None:
        return False, None
    if isinstance(deripple, dict):
        return bool(deripple.get("apply_deripple", 0)), deripple.get("filter_coeff")
    if isinstance(deripple, (tuple, list)):
        return bool(deripple[0]), deripple[1]
    if isinstance(deripple, (bool, int, np.bool_)):
        return bool(deripple), None
    return bool(getattr(deripple, "apply_deripple")), getattr(deripple, "filter_coeff", None)


class SynthesisPlan(_Plan):
    """Device plan of one inverse filter bank (tables, twiddles, scratch, carry-over)."""

    _destroy = "pfb_synthesis_plan_destroy"

    def __init__(self, n_chan: int, os_factor, input_fft_length: int, input_overlap: int = None,
                 spans_nyquist: bool = True, combine: int = 1, deripple: bool = False,
                 filter_coeff=None, temporal_taper=None, spectral_taper=None, n_pol: int = 1,
                 device: int = 0):
        super().__init__()
        self.os_factor = as_rational(os_factor)
        self.n_chan = int(n_chan)
        self.input_fft_length = int(input_fft_length)
        self.input_overlap = (self.input_fft_length // 8 if input_overlap is None
                              else int(input_overlap))
        self.n_pol = int(n_pol)
        self.device = int(device)
        nf, ov = self.input_fft_length, self.input_overlap
        tk, tco = _resolve_taper(temporal_taper, nf, ov)
        L = (nf * self.os_factor.de // self.os_factor.nu) * self.n_chan
        sk, sco = _resolve_taper(spectral_taper, nf, ov, spectral_length=L)
        taps = _taps64(filter_coeff) if filter_coeff is not None else np.zeros(1)
        self._keep = []
        tarr, tptr = _lib.c_double_array(taps)
        self._keep.append(tarr)
        tcp = sco_p = None
        if tco is not None:
            a, tcp = _lib.c_double_array(tco)
            self._keep.append(a)
        if sco is not None:
            a, sco_p = _lib.c_double_array(sco)
            self._keep.append(a)
        d = _lib.SynthesisDesc(self.n_chan, self.os_factor.nu, self.os_factor.de, nf, ov,
                               1 if spans_nyquist else 0, int(combine), 1 if deripple else 0,
                               tptr, len(tarr) if filter_coeff is not None else 0,
                               tk, tcp, sk, sco_p, self.n_pol, self.device)
        h = c_void_p()
        _lib.check(self._lib.pfb_synthesis_plan_create(byref(d), byref(h)))
        self._h = h
        W = (nf * self.os_factor.de) // self.os_factor.nu
        self.output_fft_length = W * self.n_chan
        self.output_overlap = (ov * self.os_factor.de * self.n_chan) // self.os_factor.nu
        self.output_keep = self.output_fft_length - 2 * self.output_overlap
        self.input_keep = nf - 2 * ov

    def set_chunk_blocks(self, blocks: int):
        _lib.check(self._lib.pfb_synthesis_set_chunk_blocks(self._h, int(blocks)))

    STAGE1_ROWS = {"auto": _lib.PFB_STAGE1_AUTO, "stored": _lib.PFB_STAGE1_STORED,
                   "recomputed": _lib.PFB_STAGE1_RECOMPUTED}

    def set_stage1_rows(self, mode: str):
        """Round trip only (pfb_synthesis_set_stage1_rows): 'stored' — the analysis writes
        the synthesis stage-1 rows and the synthesis reads them; 'recomputed' — the
        synthesis evaluates them from the input series (N = 256 streaming shapes;
        bit-identical output); 'auto' — the measured-faster one."""
        _lib.check(self._lib.pfb_synthesis_set_stage1_rows(self._h, self.STAGE1_ROWS[mode]))
        self._rt_input = None  # a split round trip in flight is not continued under another mode

    @property
    def last_stage1_rows(self) -> str:
        """Where the plan's last synthesis launch got its stage-1 rows ('stored',
        'recomputed'; 'none' before any launch) — pfb_synthesis_last_stage1_rows."""
        return _mode_name(self, "pfb_synthesis_last_stage1_rows", _STAGE1_NAMES)

    def output_length(self, n_dat: int) -> int:
        return int(self._lib.pfb_synthesis_output_length(self._h, int(n_dat)))

    @property
    def buffered_samples(self) -> int:
        return int(self._lib.pfb_inverse_filterbank_buffered(self._h))

    def reset(self):
        _lib.check(self._lib.pfb_inverse_filterbank_reset(self._h))

    def set_stream_sample_offset(self, sample_offset: int):
        """InverseFilterBank.sample_offset (0-based) of the stateful ``execute(...,
        stateful=True)`` calls (pfb_inverse_filterbank_set_sample_offset)."""
        _lib.check(self._lib.pfb_inverse_filterbank_set_sample_offset(self._h, int(sample_offset)))

    def _prep_in(self, x, layout: str):
        """Accept (n_pol, n_chan, n_dat) Matlab-shaped or (n_pol, n_dat, n_chan) buffers."""
        if is_device_array(x):
            t = _torch()
            x = x.to(t.complex64)
            if layout == "pfc":
                ptc = x.transpose(1, 2)
            else:
                ptc = x
            return ptc.contiguous(), True
        x = np.asarray(x)
        ptc = x.transpose(0, 2, 1) if layout == "pfc" else x
        return np.ascontiguousarray(ptc, dtype=np.complex64), False

    def _length_due(self, n_dat: int, sample_offset: int, stateful: bool) -> int:
        """Samples per polarisation a call of ``n_dat`` rows returns: a stateful call inverts
        them behind the buffered rows, a stateless one from row ``sample_offset`` (1-based)."""
        if stateful:
            return self.output_length(self.buffered_samples + n_dat)
        return self.output_length(max(n_dat - (int(sample_offset) - 1), 0))

    def _out_buffer(self, out, due: int, device, python_checks_width: bool):
        """-> (the complex64 (n_pol, width) buffer a cf32-output call writes, the capacity it
        tells the C ABI): a new buffer of ``due`` samples, or the caller's ``out=``.

        The entries differ on purpose, and tests pin each behaviour — do not unify them.
        ``execute`` (``python_checks_width``) predates the C ABI's capacity report: it refuses
        a buffer narrower than ``due`` itself, with ValueError, and passes its width on only
        when something is due (else ``due`` as it is).  ``execute_view`` and ``execute_dada``
        leave the width to the C ABI, which answers PFB_ERR_BUFFER_TOO_SMALL before it changes
        any state, and always pass it on."""
        t = _torch()
        if out is None:
            out = t.empty((self.n_pol, max(due, 0)), dtype=t.complex64, device=device)
        elif (out.dtype != t.complex64 or out.device != device or not out.is_contiguous()
              or out.dim() != 2 or out.shape[0] != self.n_pol
              or (python_checks_width and out.shape[1] < max(due, 0))):
            width = f">= {max(due, 0)}" if python_checks_width else "n"
            raise ValueError(f"out must be a contiguous complex64 ({self.n_pol}, {width}) tensor on {device}, "
                             f"got {tuple(out.shape)} {out.dtype} {out.device}")
        return out, (due if python_checks_width and due <= 0 else out.shape[1])

    def _run(self, stateful: bool, stream_fn, plan_fn, sample_offset: int, src: tuple, dst: tuple):
        """One call of a stateful / stateless pair of C ABI entries: the same arguments — the
        input's, then the output's — with ``sample_offset`` between them for the stateless
        entry only (the stream object's own is ``set_stream_sample_offset``)."""
        if stateful:
            _lib.check(stream_fn(self._h, *src, *dst))
        else:
            _lib.check(plan_fn(self._h, *src, int(sample_offset), *dst))

    def execute(self, x, sample_offset: int = 1, stateful: bool = False, layout: str = "pfc", out=None):
        """Run the synthesis; returns the (n_pol, n_out) series.  ``out``: an optional
        contiguous complex64 device buffer of at least (n_pol, output length) samples to
        write into (device input only; for graph capture without per-call allocations)."""
        ptc, dev = self._prep_in(x, layout)
        if ptc.shape[0] != self.n_pol or ptc.shape[2] != self.n_chan:
            raise ValueError(f"plan built for (n_pol={self.n_pol}, n_chan={self.n_chan}), "
                             f"got {tuple(ptc.shape)} [pol, time, chan]")
        n_dat = ptc.shape[1]
        cap = self._length_due(n_dat, sample_offset, stateful)
        if out is not None and not dev:
            raise ValueError("out= needs device input")
        if dev:
            out, cap = self._out_buffer(out, cap, ptc.device, python_checks_width=True)
            src, dst, mem, stream = c_void_p(ptc.data_ptr()), c_void_p(out.data_ptr()), \
                _lib.PFB_MEM_DEVICE, _stream_of(ptc, self)
        else:
            out = np.empty((self.n_pol, max(cap, 0)), dtype=np.complex64)
            src, dst, mem, stream = ptc.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p), \
                _lib.PFB_MEM_HOST, c_void_p(0)
        n_out = c_int64(0)
        self._run(stateful, self._lib.pfb_inverse_filterbank_execute, self._lib.pfb_synthesis_execute,
                  sample_offset, (src, n_dat * self.n_chan, n_dat), (dst, cap, cap, byref(n_out), mem, stream))
        return out[:, :n_out.value]

    def execute_dada(self, raw, nbit: int, ndim: int = 2, lowcbf: bool = False, sample_offset: int = 1,
                     stateful: bool = False, out=None):
        """The synthesis of a DADA data section (``raw``: a device tensor of bytes or
        samples, n_dat x n_chan x n_pol x ndim values of nbit in TFP or LowCBF order) —
        bit for bit ``execute(layout.dada_unpack(raw, ...), layout="ptc")``, without the
        unpacked samples crossing HBM where the channel IFFT can read the section itself
        (pfb_synthesis_execute_dada / pfb_inverse_filterbank_execute_dada;
        ``last_dada_input()`` tells).  n_dat is inferred as ``layout.dada_unpack`` does."""
        raw, n_dat = _section(raw, "execute_dada", self.n_chan * self.n_pol, nbit, ndim, lowcbf)
        out, width = self._out_buffer(out, self._length_due(n_dat, sample_offset, stateful), raw.device,
                                      python_checks_width=False)
        n_out = c_int64(0)
        self._run(stateful, self._lib.pfb_inverse_filterbank_execute_dada, self._lib.pfb_synthesis_execute_dada,
                  sample_offset, (c_void_p(raw.data_ptr()), int(nbit), int(ndim), _order(lowcbf), n_dat),
                  (c_void_p(out.data_ptr()), width, width, byref(n_out), _stream_of(raw, self)))
        return out[:, :n_out.value]

    def execute_to_dada(self, chan, out_nbit: int, scale: float = 1.0, sample_offset: int = 1,
                        stateful: bool = False, layout: str = "pfc"):
        """The synthesis of device rows ``chan`` written as a single-channel DADA data
        section: bit for bit ``layout.dada_pack(float32(scale) * execute(chan, ...), out_nbit)``
        — TFP order, NDIM 2 — without the complex float32 series crossing HBM where the
        synthesis kernel can store the samples itself (pfb_synthesis_execute_to_dada /
        pfb_inverse_filterbank_execute_to_dada; ``last_dada_output()`` tells).  Returns a
        device tensor of shape (n_out, 1, n_pol, 2), int8 / int16 / float32 / float64."""
        if not is_device_array(chan):
            raise _lib.PfbError(_lib.PFB_ERR_INVALID_ARG, "execute_to_dada: expects a device tensor")
        ptc, _ = self._prep_in(chan, layout)
        if ptc.shape[0] != self.n_pol or ptc.shape[2] != self.n_chan:
            raise ValueError(f"plan built for (n_pol={self.n_pol}, n_chan={self.n_chan}), "
                             f"got {tuple(ptc.shape)} [pol, time, chan]")
        n_dat = ptc.shape[1]
        sec, nbytes = _alloc_section((self._length_due(n_dat, sample_offset, stateful), 1, self.n_pol, 2),
                                     out_nbit, ptc.device)
        n_out = c_int64(0)
        self._run(stateful, self._lib.pfb_inverse_filterbank_execute_to_dada,
                  self._lib.pfb_synthesis_execute_to_dada, sample_offset,
                  (c_void_p(ptc.data_ptr()), n_dat * self.n_chan, n_dat),
                  (c_void_p(sec.data_ptr()), int(out_nbit), float(scale), nbytes, byref(n_out),
                   _stream_of(ptc, self)))
        return sec[:n_out.value]

    def execute_dada_to_dada(self, raw, nbit: int, out_nbit: int, scale: float = 1.0, ndim: int = 2,
                             lowcbf: bool = False, sample_offset: int = 1, stateful: bool = False):
        """``execute_dada`` written as a DADA data section like ``execute_to_dada``: file
        bytes in, file bytes out (pfb_synthesis_execute_dada_to_dada /
        pfb_inverse_filterbank_execute_dada_to_dada); ``last_dada_input()`` and
        ``last_dada_output()`` tell which sides the kernels read and wrote in place."""
        raw, n_dat = _section(raw, "execute_dada_to_dada", self.n_chan * self.n_pol, nbit, ndim, lowcbf)
        sec, nbytes = _alloc_section((self._length_due(n_dat, sample_offset, stateful), 1, self.n_pol, 2),
                                     out_nbit, raw.device)
        n_out = c_int64(0)
        self._run(stateful, self._lib.pfb_inverse_filterbank_execute_dada_to_dada,
                  self._lib.pfb_synthesis_execute_dada_to_dada, sample_offset,
                  (c_void_p(raw.data_ptr()), int(nbit), int(ndim), _order(lowcbf), n_dat),
                  (c_void_p(sec.data_ptr()), int(out_nbit), float(scale), nbytes, byref(n_out),
                   _stream_of(raw, self)))
        return sec[:n_out.value]

    def last_dada_output(self) -> str:
        """How the plan's last to-DADA call wrote its section: 'fused' (the synthesis kernel
        stored the file's own bytes), 'staged' (the cf32 series packed by a second launch),
        'none' (no such call, or a cf32-output call since) — pfb_synthesis_last_dada_output."""
        return _mode_name(self, "pfb_synthesis_last_dada_output", _DADA_OUTPUT_NAMES)

    def execute_view(self, x, sample_offset: int = 1, stateful: bool = False, out=None):
        """The synthesis of a strided view: ``x`` is any complex64 device tensor view shaped
        (n_pol, n_dat, n_chan); its strides and storage offset go to the C ABI as they are
        (``pfb_synthesis_execute_strided`` / ``pfb_inverse_filterbank_execute_strided``) and
        no ``.contiguous()`` copy is made.  Bit for bit ``execute(x.contiguous(),
        layout="ptc")``; ``last_strided_input()`` tells whether the channel IFFT read the
        view in place."""
        t = _torch()
        if not is_device_array(x) or x.dtype != t.complex64 or x.dim() != 3:
            raise _lib.PfbError(_lib.PFB_ERR_INVALID_ARG,
                                "execute_view: expects a complex64 device tensor (n_pol, n_dat, n_chan)")
        if x.shape[0] != self.n_pol or x.shape[2] != self.n_chan:
            raise ValueError(f"plan built for (n_pol={self.n_pol}, n_chan={self.n_chan}), "
                             f"got {tuple(x.shape)} [pol, time, chan]")
        n_dat = int(x.shape[1])
        out, width = self._out_buffer(out, self._length_due(n_dat, sample_offset, stateful), x.device,
                                      python_checks_width=False)
        # elements available from the view's first element to the end of its storage
        in_cap = x.untyped_storage().nbytes() // x.element_size() - x.storage_offset()
        ps, rs, cs = (int(v) for v in x.stride())
        n_out = c_int64(0)
        self._run(stateful, self._lib.pfb_inverse_filterbank_execute_strided,
                  self._lib.pfb_synthesis_execute_strided, sample_offset,
                  (c_void_p(x.data_ptr()), ps, rs, cs, in_cap, n_dat),
                  (c_void_p(out.data_ptr()), width, width, byref(n_out), _stream_of(x, self)))
        return out[:, :n_out.value]

    def last_strided_input(self) -> str:
        """How the plan's last strided call read its rows: 'in_place' (the channel IFFT
        loaded through the layout), 'staged' (copied to a packed buffer first), 'none' (no
        strided call, or a packed or DADA call since) — pfb_synthesis_last_strided_input."""
        return _mode_name(self, "pfb_synthesis_last_strided_input", _STRIDED_INPUT_NAMES)

    def last_dada_input(self) -> str:
        """How the plan's last DADA call read its section: 'fused' (the channel IFFT read
        the file's own bytes), 'staged' (unpacked first), 'none' (no DADA call, or a cf32
        call since) — pfb_synthesis_last_dada_input."""
        return _mode_name(self, "pfb_synthesis_last_dada_input", _DADA_INPUT_NAMES)


# ============================================================================ round trip
def _rt_lengths(analysis, synthesis, n_dat: int, sample_offset: int, n_pol: int = None):
    """-> (K, n_out): the rows the analysis of ``n_dat`` samples makes and the samples the
    synthesis returns from row ``sample_offset`` of them.  ``n_pol``: the polarisations of the
    call's input, which both plans must be built for (the synthesis halves have no input and
    leave the pair's agreement to the C ABI)."""
    if n_pol is not None and not (analysis.n_pol == synthesis.n_pol == n_pol):
        raise ValueError(f"plans built for n_pol={analysis.n_pol}/{synthesis.n_pol}, input of n_pol={n_pol}")
    K = analysis.output_length(int(n_dat))
    return K, synthesis._length_due(K, sample_offset, False)


def _release_rt_input(synthesis, device):
    """After a round trip's synthesis half has been enqueued on ``device``'s current stream: with
    recomputed stage-1 rows that work read the input ``roundtrip_analysis`` kept."""
    if synthesis._rt_input is not None:
        _keep_alive(synthesis, synthesis._rt_input, device)
        synthesis._rt_input = None


def roundtrip(analysis: AnalysisPlan, synthesis: SynthesisPlan, x, sample_offset: int = 1,
              chan=None, out=None):
    """Analysis -> synthesis of ``x`` (device tensor, (n_pol, n_dat) or (n_pol, 1, n_dat))
    through ``pfb_roundtrip_execute`` — the sequence of test_data_pipeline.m:114,132.

    Returns ``(chan, out)``: the full channelised product as a (n_pol, K, n_chan)
    time-major buffer and the (n_pol, n_out) synthesised series.  ``chan`` is
    bit-identical to ``analysis.execute(x)``; ``out`` equals ``synthesis.execute(chan,
    sample_offset, layout="ptc")`` bit for bit on the chunked pipeline and to ~1e-7 on
    the fused path (include/pfb_api.h, pfb_roundtrip_execute).
    ``chan``/``out`` may be preallocated buffers of the right shapes (graph capture).
    """
    x, dev = analysis._prep_in(x)
    if not dev:
        raise ValueError("roundtrip() takes device tensors (use the separate calls for host arrays)")
    n_pol, n_dat = x.shape
    K, n_out = _rt_lengths(analysis, synthesis, n_dat, sample_offset, n_pol)
    if chan is None:  # (x is complex64 on its device: _prep_in)
        chan = x.new_empty((n_pol, max(K, 0), analysis.n_chan))
    if out is None:
        out = x.new_empty((n_pol, max(n_out, 0)))
    if tuple(chan.shape) != (n_pol, K, analysis.n_chan) or tuple(out.shape) != (n_pol, n_out):
        raise ValueError("preallocated chan/out have the wrong shape")
    kr, no = c_int64(0), c_int64(0)
    _lib.check(analysis._lib.pfb_roundtrip_execute(
        analysis._h, synthesis._h, c_void_p(x.data_ptr()), n_dat, n_dat,
        c_void_p(chan.data_ptr()), K * analysis.n_chan, K, byref(kr), int(sample_offset),
        c_void_p(out.data_ptr()), max(n_out, 1), n_out, byref(no), _stream_of(x, analysis, synthesis)))
    return chan, out


def roundtrip_analysis(analysis: AnalysisPlan, synthesis: SynthesisPlan, x, sample_offset: int = 1,
                       chan=None):
    """The analysis half of the fused round trip (``pfb_roundtrip_analysis_execute``):
    writes the channelised product (returned, as ``roundtrip``'s ``chan``) and leaves the
    synthesis stage-1 rows in ``synthesis``'s scratch for ``roundtrip_synthesis``.  For
    pipelining consecutive blocks over two streams (each block on its own plan pair);
    the caller orders the halves.  ``PfbError`` (unsupported) when the plans take the
    chunked pipeline."""
    x, dev = analysis._prep_in(x)
    if not dev:
        raise ValueError("roundtrip_analysis() takes device tensors")
    n_pol, n_dat = x.shape
    K, _ = _rt_lengths(analysis, synthesis, n_dat, sample_offset, n_pol)
    if chan is None:
        chan = x.new_empty((n_pol, max(K, 0), analysis.n_chan))
    if tuple(chan.shape) != (n_pol, K, analysis.n_chan):
        raise ValueError("preallocated chan has the wrong shape")
    kr = c_int64(0)
    _lib.check(analysis._lib.pfb_roundtrip_analysis_execute(
        analysis._h, synthesis._h, c_void_p(x.data_ptr()), n_dat, n_dat,
        c_void_p(chan.data_ptr()), K * analysis.n_chan, K, byref(kr), int(sample_offset),
        _stream_of(x, analysis, synthesis)))
    # with recomputed stage-1 rows the synthesis half re-reads this input: `x` may be a
    # temporary made by _prep_in (another dtype, a non-contiguous view), so the plan keeps
    # it alive until roundtrip_synthesis has been enqueued (which records it on its stream)
    synthesis._rt_input = x
    return chan


def roundtrip_synthesis(analysis: AnalysisPlan, synthesis: SynthesisPlan, n_dat: int,
                        sample_offset: int = 1, out=None, device=None):
    """The synthesis half (``pfb_roundtrip_synthesis_execute``) of a
    ``roundtrip_analysis`` call with the same ``n_dat`` / ``sample_offset``: returns the
    (n_pol, n_out) series, equal to ``roundtrip``'s ``out`` bit for bit.  Runs on the
    current stream of ``out``'s device (or ``device``)."""
    t = _torch()
    n_pol = synthesis.n_pol
    _, n_out = _rt_lengths(analysis, synthesis, n_dat, sample_offset)
    if out is None:
        dv = t.device("cuda", synthesis.device if device is None else device)
        out = t.empty((n_pol, max(n_out, 0)), dtype=t.complex64, device=dv)
    if tuple(out.shape) != (n_pol, n_out):
        raise ValueError("preallocated out has the wrong shape")
    no = c_int64(0)
    stream = _stream_of(out, analysis, synthesis)
    _lib.check(analysis._lib.pfb_roundtrip_synthesis_execute(
        analysis._h, synthesis._h, int(n_dat), int(sample_offset), c_void_p(out.data_ptr()),
        max(n_out, 1), n_out, byref(no), stream))
    _release_rt_input(synthesis, out.device)
    return out


def roundtrip_dada(analysis: AnalysisPlan, synthesis: SynthesisPlan, raw, nbit: int, out_nbit: int,
                   scale: float = 1.0, sample_offset: int = 1, ndim: int = 2, lowcbf: bool = False):
    """The round trip from file bytes to file bytes (``pfb_roundtrip_execute_dada_to_dada``):
    ``raw`` is a device tensor holding a single-channel DADA data section ([t][pol][re, im],
    ``nbit`` 8/16/32/64).  Returns ``(chan_section, out_section)``: the channelised file's
    section, float32 of shape (K, n_chan, n_pol, 2), and the output file's section of shape
    (n_out, 1, n_pol, 2), int8 / int16 / float32 / float64, each component
    ``to_sample(float32(scale) * y)``.  Bit for bit ``layout.dada_unpack`` -> ``roundtrip`` ->
    ``layout.dada_pack`` of both results; ``analysis.last_dada_input()``,
    ``analysis.last_dada_output()`` and ``synthesis.last_dada_output()`` tell whether the
    kernels read and wrote the sections themselves."""
    n_pol = analysis.n_pol
    raw, n_dat = _section(raw, "roundtrip_dada", n_pol, nbit, ndim, lowcbf)
    K, n_out = _rt_lengths(analysis, synthesis, n_dat, sample_offset, n_pol)
    chan, chan_bytes = _alloc_section((K, analysis.n_chan, n_pol, 2), 32, raw.device)
    out, out_bytes = _alloc_section((n_out, 1, n_pol, 2), out_nbit, raw.device)
    kr, no = c_int64(0), c_int64(0)
    _lib.check(analysis._lib.pfb_roundtrip_execute_dada_to_dada(
        analysis._h, synthesis._h, c_void_p(raw.data_ptr()), int(nbit), int(ndim), _order(lowcbf), n_dat,
        c_void_p(chan.data_ptr()), chan_bytes, byref(kr), int(sample_offset),
        c_void_p(out.data_ptr()), int(out_nbit), float(scale), out_bytes, byref(no),
        _stream_of(raw, analysis, synthesis)))
    _keep_alive(synthesis, raw, raw.device)
    return chan[:kr.value], out[:no.value]


def roundtrip_analysis_dada(analysis: AnalysisPlan, synthesis: SynthesisPlan, raw, nbit: int,
                            sample_offset: int = 1, ndim: int = 2, lowcbf: bool = False):
    """The analysis half of ``roundtrip_dada`` (``pfb_roundtrip_analysis_execute_dada``):
    returns the channelised section and leaves the stage-1 rows in ``synthesis``'s scratch
    for ``roundtrip_synthesis_to_dada`` (or ``roundtrip_synthesis``).  The rows are always
    stored, so the synthesis half never comes back to ``raw``.  ``PfbError`` (unsupported)
    when the plans take the chunked pipeline."""
    n_pol = analysis.n_pol
    raw, n_dat = _section(raw, "roundtrip_analysis_dada", n_pol, nbit, ndim, lowcbf)
    K, _ = _rt_lengths(analysis, synthesis, n_dat, sample_offset, n_pol)
    chan, chan_bytes = _alloc_section((K, analysis.n_chan, n_pol, 2), 32, raw.device)
    kr = c_int64(0)
    _lib.check(analysis._lib.pfb_roundtrip_analysis_execute_dada(
        analysis._h, synthesis._h, c_void_p(raw.data_ptr()), int(nbit), int(ndim), _order(lowcbf), n_dat,
        c_void_p(chan.data_ptr()), chan_bytes, byref(kr), int(sample_offset),
        _stream_of(raw, analysis, synthesis)))
    _keep_alive(synthesis, raw, raw.device)
    return chan[:kr.value]


def roundtrip_synthesis_to_dada(analysis: AnalysisPlan, synthesis: SynthesisPlan, n_dat: int,
                                out_nbit: int, scale: float = 1.0, sample_offset: int = 1, device=None):
    """The synthesis half (``pfb_roundtrip_synthesis_execute_to_dada``) of a
    ``roundtrip_analysis_dada`` or ``roundtrip_analysis`` call with the same ``n_dat`` /
    ``sample_offset``: returns the output section, equal to ``roundtrip_dada``'s bit for bit.
    Runs on the current stream of ``device`` (default: the synthesis plan's)."""
    t = _torch()
    _, n_out = _rt_lengths(analysis, synthesis, n_dat, sample_offset)
    dv = t.device("cuda", synthesis.device if device is None else device)
    out, out_bytes = _alloc_section((n_out, 1, synthesis.n_pol, 2), out_nbit, dv)
    no = c_int64(0)
    stream = _stream_of(out, analysis, synthesis)
    _lib.check(analysis._lib.pfb_roundtrip_synthesis_execute_to_dada(
        analysis._h, synthesis._h, int(n_dat), int(sample_offset), c_void_p(out.data_ptr()),
        int(out_nbit), float(scale), out_bytes, byref(no), stream))
    _release_rt_input(synthesis, out.device)  # (a cf32 analysis half with recomputed rows)
    return out[:no.value]


# ============================================================================ helpers
def calc_output_nbins(nbins, channels, os_factor, filter_taps, input_fft_length, input_overlap):
    """calc_output_nbins.m:1-28 (same arguments: ``os_factor`` a Rational / "nu/de" / Matlab
    struct-like, ``filter_taps`` the tap COUNT): the number of samples that emerge from
    channelisation and inversion of ``nbins`` input samples.  Evaluated by the C ABI
    (``pfb_calc_output_nbins``) in Matlab's double arithmetic; integral results come
    back as int."""
    os_ = as_rational(os_factor)
    v = float(_lib.load().pfb_calc_output_nbins(int(nbins), int(channels), os_.nu, os_.de,
                                                int(filter_taps), int(input_fft_length),
                                                int(input_overlap)))
    return int(v) if v.is_integer() else v


# ============================================================================ plan cache
_PLANS = {}


def _key(*parts):
    h = hashlib.sha1()
    for p in parts:
        if isinstance(p, np.ndarray):
            h.update(p.tobytes())
        else:
            h.update(repr(p).encode())
    return h.hexdigest()


def analysis_plan(filt, block, os_factor, variant, n_pol, device=0) -> AnalysisPlan:
    taps = _taps64(filt)
    os_ = as_rational(os_factor)
    k = _key("a", taps, int(block), str(os_), variant, int(n_pol), int(device))
    p = _PLANS.get(k)
    if p is None:
        p = AnalysisPlan(taps, block, os_, variant, n_pol, device)
        _PLANS[k] = p
    return p


def synthesis_plan(n_chan, os_factor, nf, ov, spans, combine, deripple, filt, t_taper, s_taper,
                   n_pol, device=0) -> SynthesisPlan:
    os_ = as_rational(os_factor)
    tk, tco = _resolve_taper(t_taper, nf, ov)
    sk, sco = _resolve_taper(s_taper, nf, ov, spectral_length=(nf * os_.de // os_.nu) * int(n_chan))
    taps = _taps64(filt) if (deripple and filt is not None) else None
    k = _key("s", int(n_chan), str(os_), int(nf), int(ov), bool(spans), int(combine),
             bool(deripple), taps if taps is not None else "-", tk,
             tco if tco is not None else "-", sk, sco if sco is not None else "-",
             int(n_pol), int(device))
    p = _PLANS.get(k)
    if p is None:
        p = SynthesisPlan(n_chan, os_, nf, ov, spans, combine, deripple, taps, t_taper, s_taper,
                          n_pol, device)
        _PLANS[k] = p
    return p


def _device_of(x) -> int:
    if is_device_array(x):
        return x.device.index or 0
    return 0


def _pfc_view(buf):
    """(n_pol, K, N) buffer -> Matlab-shaped (n_pol, N, K) view."""
    if is_device_array(buf):
        return buf.transpose(1, 2)
    return buf.transpose(0, 2, 1)


def _npol(x) -> int:
    shape = tuple(x.shape)
    return 1 if len(shape) == 1 else int(shape[0])


# ============================================================================ functions
def _analysis_function(variant: str, doc: str, fixed: tuple = None):
    """The Matlab-shaped function of analysis ``variant``.  ``fixed``: the (block, os_factor)
    the variant always has; they become the arguments' defaults, and what is passed is ignored."""
    def fn(in_, filt, block, os_factor, verbose_=0):
        if fixed:
            block, os_factor = fixed
        plan = analysis_plan(filt, block, os_factor, variant, _npol(in_), _device_of(in_))
        return _pfc_view(plan.execute(in_))
    if fixed:
        fn.__defaults__ = fixed + (0,)
    fn.__name__ = fn.__qualname__ = variant
    fn.__doc__ = doc
    return fn


polyphase_analysis = _analysis_function(
    "polyphase_analysis",
    """polyphase_analysis.m:1-129 (Bunton).  Returns (n_pol, block, nblocks) complex64.""")
polyphase_analysis_padded = _analysis_function(
    "polyphase_analysis_padded",
    """polyphase_analysis_padded.m:1-161 (commutator).  Returns (n_pol, block, nblocks).""")
polyphase_analysis_lowcbf = _analysis_function(
    "polyphase_analysis_lowcbf",
    """polyphase_analysis_lowcbf.m:1-49 (SKA-Low CBF PST filterbank, PSTFilterbank.m).
    Returns (n_pol, 216, nblocks).  The wrapper's ``persistent do_padding`` (1536 zeros
    before the first call's data only) lives in the cached plan of these taps.""",
    fixed=(256, "4/3"))


def polyphase_synthesis(in_, input_fully_spans_Nyquist_zone, input_fft_length, os_factor,
                        deripple_=None, sample_offset_=1, input_overlap_=None,
                        temporal_taper_=None, spectral_taper_=None, combine_=1, verbose_=0):
    """polyphase_synthesis.m:1-325 (golden inversion).  Returns (n_pol, 1, n_out)."""
    nf = int(input_fft_length)
    ov = nf // 8 if input_overlap_ is None else int(input_overlap_)
    dr, filt = _resolve_deripple(deripple_)
    shape = tuple(in_.shape)
    if len(shape) != 3:
        raise ValueError("polyphase_synthesis input must be (n_pol, n_chan, n_dat)")
    if not is_device_array(in_) and not np.iscomplexobj(np.asarray(in_)):
        raise ValueError("polyphase_synthesis input data are real-valued!")
    plan = synthesis_plan(shape[1], os_factor, nf, ov, bool(input_fully_spans_Nyquist_zone),
                          int(combine_), dr, filt, temporal_taper_, spectral_taper_, shape[0],
                          _device_of(in_))
    out = plan.execute(in_, sample_offset=int(sample_offset_))
    return out[:, None, :]
