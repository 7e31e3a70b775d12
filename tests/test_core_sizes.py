"""The size, buffer and mode-name rules of the Python plan layer (core.py), on CPU tensors.

A DADA data section holds, per time sample, ``values`` numbers of NDIM components of NBIT
bits (include/pfb_api.h: [t][chan][pol][re, im], a single-channel section [t][pol][re, im]):
``values * ndim * nbit / 8`` bytes per sample, so a tensor of B bytes holds floor(B / that)
samples, and a LowCBF section only whole heaps of 32 samples.  Every expected number below
is worked out from that by hand, not with the helpers under test.
"""
from types import SimpleNamespace

import pytest
import torch

from ska_pst_dsp_model_amd import _lib
from ska_pst_dsp_model_amd.core import AnalysisPlan, SynthesisPlan
from ska_pst_dsp_model_amd.core import _alloc_section, _section_samples


# (values per sample, nbit, ndim, raw dtype, raw elements, samples)
SECTIONS = [
    (2, 8, 1, torch.uint8, 200, 100),       # 2 B per sample
    (2, 8, 2, torch.uint8, 403, 100),       # 4 B per sample, 3 B left over
    (2, 16, 1, torch.uint8, 400, 100),      # 4 B
    (2, 16, 2, torch.int16, 400, 100),      # 800 B / 8 B
    (2, 32, 1, torch.uint8, 807, 100),      # 8 B, 7 B left over
    (2, 32, 2, torch.uint8, 1600, 100),     # 16 B
    (2, 64, 1, torch.int16, 808, 101),      # 1616 B / 16 B
    (2, 64, 2, torch.uint8, 3199, 99),      # 32 B: one byte short of 100
    (16, 8, 1, torch.uint8, 1600, 100),     # 16 B
    (16, 8, 2, torch.uint8, 3231, 100),     # 32 B, 31 B left over
    (16, 16, 1, torch.int16, 1600, 100),    # 3200 B / 32 B
    (16, 16, 2, torch.uint8, 6400, 100),    # 64 B
    (16, 32, 1, torch.uint8, 6463, 100),    # 64 B, 63 B left over
    (16, 32, 2, torch.int16, 6400, 100),    # 12800 B / 128 B
    (16, 64, 1, torch.uint8, 12800, 100),   # 128 B
    (16, 64, 2, torch.int16, 12927, 100),   # 25854 B / 256 B = 100.99
]


@pytest.mark.parametrize("values,nbit,ndim,dtype,numel,samples", SECTIONS)
def test_section_length(values, nbit, ndim, dtype, numel, samples):
    raw = torch.zeros(numel, dtype=dtype)
    assert _section_samples(raw, values, nbit, ndim, False) == samples


@pytest.mark.parametrize("held,usable", [(95, 64), (96, 96), (97, 96)])
def test_section_length_lowcbf_keeps_whole_heaps(held, usable):
    raw = torch.zeros(held * 8, dtype=torch.uint8)  # 2 values x 2 components x 2 B
    assert _section_samples(raw, 2, 16, 2, True) == usable
    assert _section_samples(raw, 2, 16, 2, False) == held


@pytest.mark.parametrize("nbit,ndim", [(12, 2), (16, 3), (12, 3)])
def test_section_length_of_a_rejected_format_is_zero(nbit, ndim):
    raw = torch.zeros(4096, dtype=torch.uint8)
    assert _section_samples(raw, 2, nbit, ndim, False) == 0
    assert _section_samples(raw, 16, nbit, ndim, True) == 0


@pytest.mark.parametrize("nbit,dtype,nbytes", [(8, torch.int8, 160), (16, torch.int16, 320),
                                               (32, torch.float32, 640), (64, torch.float64, 1280)])
def test_section_allocation(nbit, dtype, nbytes):
    sec, got = _alloc_section((5, 8, 2, 2), nbit, torch.device("cpu"))
    assert tuple(sec.shape) == (5, 8, 2, 2) and sec.dtype == dtype and sec.device.type == "cpu"
    assert got == nbytes == sec.numel() * sec.element_size()


def test_section_allocation_negative_rows():
    sec, nbytes = _alloc_section((-3, 1, 2, 2), 16, torch.device("cpu"))
    assert tuple(sec.shape) == (0, 1, 2, 2) and sec.dtype == torch.int16 and nbytes == 0


def test_section_allocation_of_a_rejected_format():
    sec, nbytes = _alloc_section((5, 8, 2, 2), 12, torch.device("cpu"))
    assert tuple(sec.shape) == (0, 8, 2, 2) and sec.dtype == torch.int8 and nbytes == 0


# (class, accessor, the C ABI getter it reads, {constant: word})
MODE_NAMES = [
    (AnalysisPlan, "last_dada_input", "pfb_analysis_last_dada_input",
     {_lib.PFB_DADA_INPUT_FUSED: "fused", _lib.PFB_DADA_INPUT_STAGED: "staged"}),
    (AnalysisPlan, "last_dada_output", "pfb_analysis_last_dada_output",
     {_lib.PFB_DADA_OUTPUT_FUSED: "fused", _lib.PFB_DADA_OUTPUT_STAGED: "staged"}),
    (SynthesisPlan, "last_dada_input", "pfb_synthesis_last_dada_input",
     {_lib.PFB_DADA_INPUT_FUSED: "fused", _lib.PFB_DADA_INPUT_STAGED: "staged"}),
    (SynthesisPlan, "last_dada_output", "pfb_synthesis_last_dada_output",
     {_lib.PFB_DADA_OUTPUT_FUSED: "fused", _lib.PFB_DADA_OUTPUT_STAGED: "staged"}),
    (SynthesisPlan, "last_strided_input", "pfb_synthesis_last_strided_input",
     {_lib.PFB_STRIDED_INPUT_IN_PLACE: "in_place", _lib.PFB_STRIDED_INPUT_STAGED: "staged"}),
    (SynthesisPlan, "last_stage1_rows", "pfb_synthesis_last_stage1_rows",
     {_lib.PFB_STAGE1_STORED: "stored", _lib.PFB_STAGE1_RECOMPUTED: "recomputed"}),
]


@pytest.mark.parametrize("cls,accessor,getter,words", MODE_NAMES,
                         ids=[f"{m[0].__name__}.{m[1]}" for m in MODE_NAMES])
def test_mode_names(cls, accessor, getter, words):
    """Each ``last_*`` accessor names what its C ABI getter reports (the getter is stubbed:
    no device is needed); 0 — the *_NONE constants, PFB_STAGE1_AUTO — and -1 are 'none'."""
    assert sorted(words) == [1, 2]

    def name_of(mode):
        handle = object()
        lib = SimpleNamespace(**{getter: lambda h: mode if h is handle else None})
        plan = SimpleNamespace(_lib=lib, _h=handle)
        member = getattr(cls, accessor)
        return member.fget(plan) if isinstance(member, property) else member(plan)

    for mode, word in words.items():
        assert name_of(mode) == word
    assert name_of(0) == "none" and name_of(-1) == "none"
