"""Stream-object surface: Channelizer / DeChannelizer / FilterBank / InverseFilterBank
and the two-stage cascades (matlab/Channelizer.m, DeChannelizer.m, FilterBank.m,
InverseFilterBank.m, TwoStageFilterBank.m, TwoStageInverseFilterBank.m).

``execute`` keeps the Matlab calling convention ``[obj, out] = execute(obj, in)``:
it returns ``(self, out)``.  The carry-over state (``FilterBank.m:13-14``) lives in
the device plan (``pfb_filterbank_execute`` / ``pfb_inverse_filterbank_execute``).
"""
from __future__ import annotations

import abc

import numpy as np

from . import layout
from .config import as_rational
from .core import AnalysisPlan, SynthesisPlan, _npol, _pfc_view, is_device_array
from .firio import read_fir_filter_coeff
from .window import PFBWindow, identity_taper

__all__ = ["Channelizer", "DeChannelizer", "FilterBank", "InverseFilterBank",
           "TwoStageFilterBank", "TwoStageInverseFilterBank"]


def _cfg(config, name, default=None):
    if isinstance(config, dict):
        return config.get(name, default)
    return getattr(config, name, default)


def _taps_from_config(config):
    taps = _cfg(config, "filt_coeff")
    if taps is None:
        taps = read_fir_filter_coeff(_cfg(config, "fir_filter_path"))
    return np.asarray(taps, dtype=np.float64).ravel()


class Channelizer(abc.ABC):
    """Channelizer.m:1-12 — abstract ``[obj, output] = execute(obj, input)``."""

    @abc.abstractmethod
    def execute(self, input):  # noqa: A002
        ...


class DeChannelizer(abc.ABC):
    """DeChannelizer.m:1-12 — abstract ``[obj, output] = execute(obj, input)``."""

    @abc.abstractmethod
    def execute(self, input):  # noqa: A002
        ...


def _to_device(x, device):
    """(array, was_host): host arrays go to the plan's device (torch as allocator)."""
    if is_device_array(x):
        return x, False
    import torch
    arr = np.ascontiguousarray(np.asarray(x), dtype=np.complex64)
    return torch.from_numpy(arr).to(torch.device("cuda", int(device))), True


def _to_host(x):
    return x.cpu().numpy()


def _quantize(x, rms, device=0):
    """round(rms / std(x) * x) (FilterBank.m:75-83,106-113) through pfb_quantize."""
    xd, host = _to_device(x, device)
    y = layout.quantize(xd, rms)
    return _to_host(y) if host else y


class FilterBank(Channelizer):
    """FilterBank.m:1-130 — analysis PFB with input buffering and nu-trimming."""

    def __init__(self, config=None, n_pol: int = None, device: int = 0, fused_quantiser: bool = None,
                 fused_input_quantiser: bool = None):
        self.pfb_analysis = "polyphase_analysis"
        self.os_factor = None
        self.filt_coeff = None
        self.n_chan = None
        self.rndInput = False
        self.rmsInput = 0.0
        self.rndOutput = False
        self.rmsOutput = 0.0
        # opt-in: the to-DADA calls take the output quantiser through the plan's quantised
        # calls (AnalysisPlan.execute_quantised_to_dada) instead of the execute fallback
        self.fused_quantiser = False
        # opt-in: ``rndInput`` is taken by the plan's input quantiser
        # (AnalysisPlan.set_input_quantiser, rms = rmsInput) on every execute entry, instead of
        # pfb_quantize into a fresh buffer and the fallbacks that follow from it
        self.fused_input_quantiser = False
        self.device = device
        self._plan = None
        self._n_pol = n_pol
        if config is not None:
            self.pfb_analysis = _cfg(config, "analysis_function", "polyphase_analysis")
            self.filt_coeff = _taps_from_config(config)
            self.n_chan = int(_cfg(config, "channels", _cfg(config, "n_chan")))
            self.os_factor = as_rational(_cfg(config, "os_factor"))
            self.rndInput = bool(_cfg(config, "rndInput", False))
            self.rmsInput = float(_cfg(config, "rmsInput", 0.0))
            self.rndOutput = bool(_cfg(config, "rndOutput", False))
            self.rmsOutput = float(_cfg(config, "rmsOutput", 0.0))
            self.fused_quantiser = bool(_cfg(config, "fused_quantiser", False))
            self.fused_input_quantiser = bool(_cfg(config, "fused_input_quantiser", False))
        if fused_quantiser is not None:
            self.fused_quantiser = bool(fused_quantiser)
        if fused_input_quantiser is not None:
            self.fused_input_quantiser = bool(fused_input_quantiser)

    def _input_fused(self) -> bool:
        """``rndInput`` goes through the plan's input quantiser: opted in and configured."""
        return bool(self.fused_input_quantiser and self.rndInput)

    def _input_fallback(self) -> bool:
        """``rndInput`` is configured and takes ``_quantize`` on the input (no opt-in)."""
        return bool(self.rndInput and not self._input_fused())

    def _quantiser_fused(self) -> bool:
        """The to-DADA calls take the plan's quantised calls: opted in, the output quantiser
        configured and no input quantiser outside the plan (whose scale needs the whole input
        first; with ``fused_input_quantiser`` the plan takes it in the same call)."""
        return bool(self.fused_quantiser and self.rndOutput and not self._input_fallback())

    def _ensure_plan(self, n_pol):
        if self._plan is None or self._plan.n_pol != n_pol:
            if self._plan is not None and self._plan.buffered_samples:
                raise ValueError("n_pol changed while samples are buffered")
            self._plan = AnalysisPlan(self.filt_coeff, self.n_chan, self.os_factor,
                                      self.pfb_analysis, n_pol, self.device)
        # (host-side state of the plan: takes effect at the next call)
        self._plan.set_input_quantiser(self.rmsInput if self._input_fused() else None)
        return self._plan

    @property
    def buffered_samples(self) -> int:
        return 0 if self._plan is None else self._plan.buffered_samples

    def execute(self, input):  # noqa: A002
        x = input
        if self._input_fallback():
            x = _quantize(x, self.rmsInput, self.device)
        plan = self._ensure_plan(_npol(x))
        out = plan.execute(x, stateful=True)  # (n_pol, T_out, n_chan)
        if self.rndOutput:
            out = _quantize(out, self.rmsOutput, self.device)
        return self, _pfc_view(out)

    def execute_dada(self, raw, nbit: int, ndim: int = 2, n_pol: int = 1):
        """``execute`` of the next chunk as the file holds it: ``raw`` is a device tensor of
        a single-channel DADA section's bytes (``DADARead.generate_raw``), ``n_pol``
        polarisations interleaved (TFP).  Same output and carry as
        ``execute(DADARead.generate(...)[:, 0, :])``, bit for bit
        (``AnalysisPlan.execute_dada``).  With ``rndInput`` set the section is unpacked and
        takes ``execute``: the quantiser's scale needs the variance of the whole input — unless
        ``fused_input_quantiser`` is set: the plan's input quantiser then takes the moments of
        the section where it lies and the kernel rounds as it loads."""
        if self._input_fallback():
            x = layout.dada_unpack(raw, nbit, ndim, 1, int(n_pol))[:, :, 0]
            return self.execute(x)
        plan = self._ensure_plan(int(n_pol))
        out = plan.execute_dada(raw, nbit, ndim=ndim, stateful=True)  # (n_pol, T_out, n_chan)
        if self.rndOutput:
            out = _quantize(out, self.rmsOutput, self.device)
        return self, out.transpose(1, 2)

    def execute_to_dada(self, input, nbit: int, scale: float = 1.0):  # noqa: A002
        """``execute`` of the next chunk (device series) written as a DADA data section:
        returns ``(self, section)`` with ``section`` the (T_out, n_chan, n_pol, 2) device
        tensor of int8 / int16 / float32 / float64 samples (TFP order), bit for bit
        ``layout.dada_pack(float32(scale) * out, nbit)`` of ``execute``'s engine-order
        output, and the same carry (``AnalysisPlan.execute_to_dada``).  With ``rndInput``,
        ``rndOutput`` or ``rmsOutput`` configured the quantiser's scale needs the variance of
        the whole input or output (FilterBank.m:75-83,106-113): the call then takes
        ``execute`` followed by ``layout.dada_pack`` — unless ``fused_quantiser`` is set, which
        sends the ``rndOutput`` case (without ``rndInput``) through
        ``AnalysisPlan.execute_quantised_to_dada`` with ``rms = rmsOutput``: the moments summed
        by the analysis kernel, one pass over the product.  With ``fused_input_quantiser``
        ``rndInput`` is the plan's input quantiser and causes no fallback."""
        if self._quantiser_fused():
            plan = self._ensure_plan(_npol(input))
            return self, plan.execute_quantised_to_dada(input, nbit, self.rmsOutput, scale=scale, stateful=True)
        if self._input_fallback() or self.rndOutput or self.rmsOutput:
            _, view = self.execute(input)
            return self, self._pack_view(view, nbit, scale)
        plan = self._ensure_plan(_npol(input))
        return self, plan.execute_to_dada(input, nbit, scale=scale, stateful=True)

    def execute_dada_to_dada(self, raw, in_nbit: int, out_nbit: int, scale: float = 1.0, ndim: int = 2,
                             n_pol: int = 1):
        """``execute_dada`` written as a DADA data section like ``execute_to_dada``: file
        bytes in, file bytes out (``AnalysisPlan.execute_dada_to_dada``), with the same
        fallbacks for the quantisation hooks (and the same ``fused_quantiser`` path)."""
        if self._quantiser_fused():
            plan = self._ensure_plan(int(n_pol))
            return self, plan.execute_dada_quantised_to_dada(raw, in_nbit, out_nbit, self.rmsOutput, scale=scale,
                                                             ndim=ndim, stateful=True)
        if self._input_fallback() or self.rndOutput or self.rmsOutput:
            _, view = self.execute_dada(raw, in_nbit, ndim=ndim, n_pol=n_pol)
            return self, self._pack_view(view, out_nbit, scale)
        plan = self._ensure_plan(int(n_pol))
        return self, plan.execute_dada_to_dada(raw, in_nbit, out_nbit, scale=scale, ndim=ndim, stateful=True)

    @staticmethod
    def _pack_view(view, nbit, scale):
        """The (n_pol, n_chan, T) view ``execute`` returns -> the scaled, packed section."""
        import torch
        buf = view.transpose(1, 2).contiguous()  # engine (n_pol, T, n_chan) order
        if float(scale) != 1.0:
            # (per component, in float32: not a complex product)
            buf = torch.view_as_complex(torch.view_as_real(buf) * float(scale))
        sec = layout.dada_pack(buf, nbit)
        return sec.reshape(buf.shape[1], buf.shape[2], buf.shape[0], 2)

    def reset(self):
        if self._plan is not None:
            self._plan.reset()


class InverseFilterBank(DeChannelizer):
    """InverseFilterBank.m:1-139 — synthesis with input buffering.

    The Matlab object forces ``deripple = false`` before every call
    (InverseFilterBank.m:90); ``honour_deripple=True`` applies the configured value
    instead (used by the test pipeline, which calls polyphase_synthesis directly with
    deripple on, test_data_pipeline.m:132)."""

    def __init__(self, config=None, device: int = 0, honour_deripple: bool = False):
        self.os_factor = as_rational("1/1")
        self.filt_coeff = None
        self.nchan = None
        self.n_fft = None
        self.overlap = None
        self.sample_offset = 0
        self.temporal_taper = None
        self.spectral_taper = identity_taper
        self.deripple = False
        self.critical = False
        self.combine = 1
        self.window_factory = PFBWindow()
        self.device = device
        self.honour_deripple = honour_deripple
        self._plan = None
        self._plan_key = None
        if config is not None:
            self.filt_coeff = _taps_from_config(config)
            self.n_fft = int(_cfg(config, "input_fft_length"))
            self.nchan = int(_cfg(config, "channels", _cfg(config, "n_chan")))
            self.os_factor = as_rational(_cfg(config, "os_factor"))
            self.overlap = int(_cfg(config, "input_overlap"))
            self.deripple = bool(_cfg(config, "deripple", False))
            factory = self.window_factory.lookup[_cfg(config, "temporal_taper", "no_window")]
            self.temporal_taper = factory(self.n_fft, self.overlap)

    def frequency_taper(self, name):
        """InverseFilterBank.m:48-61."""
        factory = self.window_factory.lookup[name]
        self.spectral_taper = factory(self.n_fft, self.overlap)
        return self

    def _ensure_plan(self, n_pol, n_chan):
        spans = not self.critical  # :89
        dr = self.deripple if self.honour_deripple else False  # :90
        key = (n_pol, n_chan, spans, dr, self.combine, id(self.temporal_taper),
               id(self.spectral_taper))
        if self._plan is None or key != self._plan_key:
            if self._plan is not None and self._plan.buffered_samples:
                raise ValueError("configuration changed while samples are buffered")
            self._plan = SynthesisPlan(n_chan, self.os_factor, self.n_fft, self.overlap, spans,
                                       self.combine, dr, self.filt_coeff, self.temporal_taper,
                                       self.spectral_taper, n_pol, self.device)
            self._plan_key = key
        return self._plan

    @property
    def buffered_samples(self) -> int:
        return 0 if self._plan is None else self._plan.buffered_samples

    def _stream_plan(self, n_pol, n_chan):
        """Every call's preamble: the plan of this shape, told the object's ``sample_offset``
        — polyphase_synthesis(..., obj.sample_offset+1, ...) on every call (:92-96)."""
        if int(self.sample_offset) < 0:
            raise ValueError("sample_offset is 0-based (>= 0)")
        plan = self._ensure_plan(n_pol, n_chan)
        plan.set_stream_sample_offset(int(self.sample_offset))
        return plan

    def execute(self, input):  # noqa: A002
        shape = tuple(input.shape)
        if not is_device_array(input) and not np.iscomplexobj(np.asarray(input)):
            raise ValueError("polyphase_synthesis input data are real-valued!")
        out = self._stream_plan(shape[0], shape[1]).execute(input, stateful=True)
        return self, out[:, None, :]

    def execute_view(self, view):
        """``execute`` of the next chunk read where it lies: ``view`` is a complex64 device
        tensor view in engine order (n_pol, n_dat, n_chan) with any positive strides (the
        coarse-channel slices of a two-stage product, a channel window, channel-major
        rows).  Same output and carry as ``execute(view.transpose(1, 2))``, bit for bit,
        with no packed copy of the view (``SynthesisPlan.execute_view``)."""
        plan = self._stream_plan(int(view.shape[0]), int(view.shape[2]))
        out = plan.execute_view(view, stateful=True)
        return self, out[:, None, :]

    def execute_dada(self, raw, nbit: int, ndim: int = 2, lowcbf: bool = False, n_pol: int = 1):
        """``execute`` of the next chunk as the file holds it: ``raw`` is a device tensor of
        the DADA section's bytes (``DADARead.generate_raw``), ``nchan`` channels x ``n_pol``
        polarisations.  Same output and carry as ``execute(DADARead.generate(...))``."""
        plan = self._stream_plan(int(n_pol), int(self.nchan))
        out = plan.execute_dada(raw, nbit, ndim=ndim, lowcbf=lowcbf, stateful=True)
        return self, out[:, None, :]

    def _quantised_output(self) -> bool:
        # (InverseFilterBank.m has no output quantiser; an object given FilterBank's
        # rndOutput / rmsOutput hooks packs what ``execute`` returns, as FilterBank does: a
        # quantiser needs the variance of the whole output)
        return bool(getattr(self, "rndOutput", False) or getattr(self, "rmsOutput", 0.0))

    @staticmethod
    def _pack_out(out, nbit, scale):
        """The (n_pol, 1, n_out) series ``execute`` returns -> the scaled, packed section."""
        import torch
        buf = out[:, 0, :].contiguous()[:, :, None]  # (n_pol, n_out, 1 channel)
        if float(scale) != 1.0:
            # (per component, in float32: not a complex product)
            buf = torch.view_as_complex(torch.view_as_real(buf) * float(scale))
        return layout.dada_pack(buf, nbit).reshape(buf.shape[1], 1, buf.shape[0], 2)

    def execute_to_dada(self, input, nbit: int, scale: float = 1.0):  # noqa: A002
        """``execute`` of the next chunk (device rows) written as a single-channel DADA data
        section: returns ``(self, section)`` with ``section`` the (n_out, 1, n_pol, 2) device
        tensor of int8 / int16 / float32 / float64 samples (TFP order), bit for bit
        ``layout.dada_pack(float32(scale) * out, nbit)`` of ``execute``'s output, and the same
        carry (``SynthesisPlan.execute_to_dada``)."""
        if self._quantised_output():
            _, out = self.execute(input)
            return self, self._pack_out(out, nbit, scale)
        shape = tuple(input.shape)
        plan = self._stream_plan(shape[0], shape[1])
        return self, plan.execute_to_dada(input, nbit, scale=scale, stateful=True)

    def execute_dada_to_dada(self, raw, in_nbit: int, out_nbit: int, scale: float = 1.0, ndim: int = 2,
                             lowcbf: bool = False, n_pol: int = 1):
        """``execute_dada`` written as a DADA data section like ``execute_to_dada``: file
        bytes in, file bytes out (``SynthesisPlan.execute_dada_to_dada``)."""
        if self._quantised_output():
            _, out = self.execute_dada(raw, in_nbit, ndim=ndim, lowcbf=lowcbf, n_pol=n_pol)
            return self, self._pack_out(out, out_nbit, scale)
        plan = self._stream_plan(int(n_pol), int(self.nchan))
        return self, plan.execute_dada_to_dada(raw, in_nbit, out_nbit, scale=scale, ndim=ndim, lowcbf=lowcbf,
                                               stateful=True)

    def reset(self):
        if self._plan is not None:
            self._plan.reset()


class TwoStageFilterBank(Channelizer):
    """TwoStageFilterBank.m:1-118 — stage 2 cascaded over every stage-1 channel (pol 1).

    The Matlab object runs nch1 independent FilterBank objects in a loop (:92-110).
    Here stage 2 is ONE batched plan whose "polarisations" are the nch1 stage-1
    channels (each keeps its own carry-over, as the separate objects do).  Stage 1
    writes its product channel-major, so pol 1's channels are the stage-2 series as
    they lie, and the batched stage 2 writes the assembled output with the oversampled
    channels chomped out (:102-105) straight from its FFT
    (``pfb_filterbank_execute_strided``: the streaming-kernel shapes of
    ``polyphase_analysis`` and every ``polyphase_analysis_padded`` plan, whose strided call
    also drops the rows [T_out, K) of the circular shift at the store).  A stage that does
    not store strided takes a corner turn (``pfb_corner_turn``, stage 1) or a gather
    (``pfb_gather_channels``, stage 2): stages whose plan has no strided store, all of them
    with ``strided = False``, and the stages ``_STRIDED_DEFAULT`` leaves on that path.  Every
    combination computes the same values, bit for bit."""

    # (stage 1 channel-major, stage 2 assembled + chomped) by default, per analysis function:
    # the measured-faster path of each stage (profiles/twostage_strided_padded_ab.jsonl)
    _STRIDED_DEFAULT = {"padded": (True, True), "other": (True, True)}

    def __init__(self, config, device: int = 0):
        # (the stages' input quantiser stays pfb_quantize: the batched stage-2 plan's variance
        # would run over all its series at once)
        self.stage1 = FilterBank(config, device=device, fused_input_quantiser=False)
        self.config1 = config
        self.config2 = config
        self.nch1 = int(_cfg(config, "channels"))
        self.nch2 = int(_cfg(config, "channels"))
        self.critical = 0
        self.single = 0
        self.built = False
        self.stage2 = None
        self.device = device
        # both stages through pfb_filterbank_execute_strided where the kernels allow it
        # (no corner turn, no gather); False: the corner-turn / gather path
        self.strided = True
        # A/B runs: (stage 1, stage 2) True / False forces that stage's strided store on or
        # off; None: the default (_stage_strided)
        self.strided_stages = [None, None]

    def set_stage2_config(self, config):
        self.config2 = config
        self.nch2 = int(_cfg(config, "channels"))
        return self

    def build(self):
        self.stage2 = FilterBank(self.config2, device=self.device, fused_input_quantiser=False)
        self.built = True
        return self

    def execute(self, input):  # noqa: A002
        x, host = _to_device(input, self.device)
        if not self.built:
            self.build()
        view = self._execute_strided(x) if self.strided else None
        if view is None:
            series, nch1 = self._stage1_turned(x)
            view = self._stage2(series, nch1)
        return self, (_to_host(view) if host else view)

    def _stage1_turned(self, x):
        """Stage 1 through the contiguous call, then the corner turn: the (nch1, T1)
        per-channel series of pol 1."""
        _, out1 = self.stage1.execute(x)      # (n_pol, nch1, T1) view
        nch1 = 1 if self.single == 1 else self.stage1.n_chan
        # per-channel series of pol 1: (T1, nch1) rows -> (nch1, T1)
        rows = out1[0].transpose(0, 1)[:, :nch1]  # (T1, nch1) view of the engine buffer
        return layout.corner_turn(rows), nch1

    def _stage_strided(self, stage: int) -> bool:
        """Does ``stage`` (1 or 2) store strided?  ``strided_stages[stage - 1]`` when it is
        set (A/B runs), else the measured default for the stage's analysis function
        (``_STRIDED_DEFAULT``)."""
        forced = self.strided_stages[stage - 1]
        if forced is not None:
            return bool(forced)
        fb = self.stage1 if stage == 1 else self.stage2
        padded = fb.pfb_analysis in ("polyphase_analysis_padded", "padded")
        return self._STRIDED_DEFAULT["padded" if padded else "other"][stage - 1]

    def _chomp(self):
        """(nch2 kept per stage-2 bank, dropped-bin count) of :81-85,102-105."""
        os_ = self.stage1.os_factor
        nch2_orig = self.stage2.n_chan
        nch2 = (nch2_orig * os_.de) // os_.nu if self.critical else nch2_orig
        return nch2, nch2_orig - nch2

    def _stage2(self, series, nch1):
        """Stage 2 over the (nch1, T1) series, then one gather assembles the output."""
        nch2, offset = self._chomp()
        _, tmp = self.stage2.execute(series)      # (nch1, nch2_orig, T2) view
        buf2 = tmp.transpose(1, 2)                # (nch1, T2, nch2_orig) engine buffer
        T2 = int(buf2.shape[1])
        import torch
        out = torch.empty((1, T2, nch1 * nch2), dtype=torch.complex64, device=buf2.device)
        # out[t][ich*nch2 + j] = tmp[ich][t][j (+ offset from j = nch2/2 - 1 on)]
        layout.gather_channels(buf2, n_outer=nch1, in_outer_stride=buf2.stride(0),
                               in_row_stride=buf2.stride(1), n_rows=T2, n_sel=nch2,
                               split=nch2 // 2 - 1, shift=offset, out=out,
                               out_outer_stride=nch2, out_row_stride=nch1 * nch2)
        return out.transpose(1, 2)                # (1, nch1*nch2, T2)

    def _execute_strided(self, x):
        """Both stages through pfb_filterbank_execute_strided: stage 1 writes its product
        channel-major, so pol 1's channels are already the stage-2 series (no corner
        turn), and stage 2 writes the assembled, chomped output (no gather).  Same
        kernels and arithmetic as the corner-turn / gather path (bit-identical).  Padded
        stages: the strided call stores only the T_out rows it returns (the rows [T_out, K)
        of the padded variant's circular shift are dropped at the store, not written as
        scratch).  None when stage 1 cannot take this path (its plan state is then
        untouched); a stage 2 that cannot takes the gather path.  A stage ``_stage_strided``
        turns off takes its corner turn / gather while the other stays strided."""
        from ._lib import PFB_ERR_UNSUPPORTED, PfbError
        s1, s2 = self.stage1, self.stage2
        if s1.rndInput or s1.rndOutput or s2.rndInput or s2.rndOutput:
            return None
        use1, use2 = self._stage_strided(1), self._stage_strided(2)
        if not (use1 or use2):
            return None
        import torch
        if use1:
            p1 = s1._ensure_plan(_npol(x))
            xs, _ = p1._prep_in(x)
            T1 = p1.stream_rows(int(xs.shape[1]))
            nch1_all = p1.out_chan
            T1c = max(16, (T1 + 15) // 16 * 16)  # 128-B aligned channel runs
            ser = torch.empty((p1.n_pol, nch1_all, T1c), dtype=torch.complex64, device=xs.device)
            try:
                T1 = p1.execute_strided(xs, ser, nch1_all * T1c, 1, T1c)
            except PfbError as e:
                if e.status == PFB_ERR_UNSUPPORTED:
                    return None
                raise
            nch1 = 1 if self.single == 1 else nch1_all
            series = ser[0, :nch1, :T1]               # (nch1, T1), unit sample stride
        else:
            series, nch1 = self._stage1_turned(x)
            T1 = int(series.shape[1])
        if not use2:
            return self._stage2(series, nch1)
        nch2, offset = self._chomp()
        p2 = s2._ensure_plan(nch1)
        T2 = p2.stream_rows(T1)
        out = torch.empty((1, max(T2, 1), nch1 * nch2), dtype=torch.complex64, device=series.device)
        try:
            T2 = p2.execute_strided(series, out, nch2, nch1 * nch2, 1,
                                    (nch2 // 2 - 1, offset, nch2))
        except PfbError as e:
            if e.status == PFB_ERR_UNSUPPORTED:
                return self._stage2(series, nch1)
            raise
        return out[:, :T2, :].transpose(1, 2)     # (1, nch1*nch2, T2)


class TwoStageInverseFilterBank(DeChannelizer):
    """TwoStageInverseFilterBank.m:1-159 — stage-2 inversion per output coarse channel.

    The nch_out InverseFilterBank objects of the Matlab loop (:124-151) become ONE
    batched synthesis plan over nch_out "polarisations" and one synthesis call inverts
    them all.  The nch_in = nch2 * combine fine channels of coarse channel o are channels
    [o nch_in, (o + 1) nch_in) of every input row.  ``strided_input``: the plan reads them
    where they lie, as the (nch_out, T, nch_in) view with strides (nch_in, nchan, 1)
    (``pfb_inverse_filterbank_execute_strided``; a spectral taper goes through that call's
    staged path); otherwise one gather (``pfb_gather_channels``) copies the slices into
    [coarse][t][nch_in] first.  Both compute the same values, bit for bit."""

    # strided input by default, per shape class: "narrow" = slices shorter than a 128-B line
    # (nch_in < 16: neighbouring coarse channels share lines), "wide" = the rest.  True only
    # where it measured faster than the gather by more than the gather's own spread: both
    # did, the SKA-Mid inverse 4096 x 14 and the 256 x 256 cascade (DESIGN.md §6,
    # profiles/twostage_inverse_strided_ab.jsonl)
    _STRIDED_INPUT_DEFAULT = {"narrow": True, "wide": True}

    def _use_strided_input(self, nch_in: int) -> bool:
        if self.strided_input is not None:
            return bool(self.strided_input)
        return self._STRIDED_INPUT_DEFAULT["narrow" if nch_in < 16 else "wide"]

    def __init__(self, config, device: int = 0):
        # True / False: read the coarse-channel slices in place / gather them first (A/B
        # runs); None: the measured default of the shape class (_STRIDED_INPUT_DEFAULT)
        self.strided_input = None
        self.config1 = config
        self.config2 = config
        self.stage1 = InverseFilterBank(config, device=device)
        self.nch1 = int(_cfg(config, "channels"))
        self.nch2 = int(_cfg(config, "channels"))
        self.single = 0
        self.combine = 1
        self.built = False
        self.stage2 = None
        self._ftaper = None
        self.device = device

    def set_stage2_config(self, config):
        self.config2 = config
        self.nch2 = int(_cfg(config, "channels"))
        return self

    def build(self):
        self.stage2 = InverseFilterBank(self.config2, device=self.device)
        if self._ftaper is not None:
            self.stage2.frequency_taper(self._ftaper)
        self.built = True
        return self

    def frequency_taper(self, name):
        self._ftaper = name
        if not self.built:
            self.build()
        self.stage2.frequency_taper(name)
        return self

    def execute(self, input):  # noqa: A002
        import torch
        if not self.built:
            self.build()
        x, host = _to_device(input, self.device)
        if not x.is_complex():
            raise ValueError("input data are real !")
        os_ = self.stage1.os_factor
        npol, nchan, T = (int(v) for v in x.shape)
        nch_out = nchan // self.nch2
        stage2_nchan = self.stage2.nchan
        critical_stage2_nchan = (stage2_nchan * os_.de) // os_.nu
        if self.nch2 == critical_stage2_nchan:
            critical = True
        elif self.nch2 == stage2_nchan:
            critical = False
            if self.combine > 1:
                raise ValueError("TwoStageInverseFilterBank::execute cannot combine "
                                 "oversampled coarse channels")
        else:
            raise ValueError("TwoStageInverseFilterBank::execute invalid nchan")
        nch_in = self.nch2 * self.combine
        nch_out = nch_out // self.combine
        if self.single:
            nch_out = 1
        buf = x.transpose(1, 2)                   # (npol, T, nchan) engine order
        if buf.stride(2) != 1:
            buf = buf.contiguous()
        if buf.dtype != torch.complex64:
            buf = buf.to(torch.complex64)
        st = self.stage2
        st.critical = critical
        st.combine = self.combine
        if self._use_strided_input(nch_in):
            # coarse channel o = channels [o nch_in, (o + 1) nch_in) of every row, read where
            # they lie: (nch_out, T, nch_in) with strides (nch_in, row stride, 1)
            rows = buf[0][:, :nch_out * nch_in]
            view = rows.unflatten(1, (nch_out, nch_in)).permute(1, 0, 2)
            _, tmp = st.execute_view(view)            # (nch_out, 1, T_out)
        else:
            sliced = layout.gather_channels(buf[0], n_outer=nch_out, in_outer_stride=nch_in,
                                            in_row_stride=buf.stride(1), n_rows=T, n_sel=nch_in)
            _, tmp = st.execute(sliced.transpose(1, 2))  # (nch_out, 1, T_out)
        out = tmp.reshape(1, nch_out, tmp.shape[2])
        return self, (_to_host(out) if host else out)
