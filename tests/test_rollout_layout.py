"""CPU-side checks of VTAMIQ.forward_rollout: the entry points are declared, exported and bound, the header states the extents of the two
outputs, DESIGN.md names the new kernels, and the Python-level refusals come before any library call."""
import ctypes
import os
import re

import pytest
import torch

from vtamiq_amd import VTAMIQ, Rollout, _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"vtq_forward_rollout": 13, "vtq_forward_rollout_tokens": 13, "vtq_rollout_workspace_bytes": 3}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbols_are_declared_exported_and_bound():
    build.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _read("include", "vtamiq_hip.h")
    for name, nargs in ENTRIES.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    unit = _read("include", "vtamiq_hip_rollout.h")
    decl = re.search(r"\bvtq_k_rollout_step\s*\(([^;]*?)\)\s*;", unit, re.S)
    assert decl and len(decl.group(1).split(",")) == 12 == len(_lib.ROLLOUT_SIGNATURES["vtq_k_rollout_step"][1])
    assert hasattr(lib, "vtq_k_rollout_step")
    assert set(re.findall(r"\b(vtq_[a-z0-9_]+)\s*\(", unit)) - {"vtq_k_attention_probs"} >= {"vtq_k_rollout_step"}
    bound = _lib.load()
    assert bound.vtq_forward_rollout.argtypes == _lib.SIGNATURES["vtq_forward_rollout"][1]
    assert bound.vtq_k_rollout_step.argtypes == _lib.ROLLOUT_SIGNATURES["vtq_k_rollout_step"][1]
    # symbols are only added: the ABI number stays
    assert int(re.search(r"#define\s+VTQ_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == _lib.ABI_VERSION


def test_header_states_both_extents():
    hdr = _read("include", "vtamiq_hip.h")
    doc = hdr[hdr.index("ATTENTION ROLLOUT"):hdr.index("vtq_rollout_workspace_bytes(vtq_handle")]
    assert re.search(r"rollout_out\s*:\s*fp32, EXACTLY 2 \* B \* S floats", doc)
    assert re.search(r"last_attention_out\s*:\s*fp32, EXACTLY 2 \* B \* h \* S floats.*may be NULL", doc)
    unit = _read("include", "vtamiq_hip_rollout.h")
    assert "exactly nseq * S floats" in unit and "nseq * (H / 64) * ceil(S / 128) * S floats" in unit


def test_design_names_the_new_kernels():
    design = _read("DESIGN.md")
    sec0 = design[design.index("## 0."):design.index("## 1.")]
    for k in ("rollout_step_kernel", "rollout_combine_kernel", "attention_rollout.hip"):
        assert k in sec0, k
    assert "attention_rollout.hip" in build.SOURCES


def _model():
    m = VTAMIQ(vit_config=dict(variant="ViT-B16", num_keep_layers=1, pretrained=False), calibrate=False, precision="fp16x3").eval()

    def no_library():
        raise AssertionError("the library was reached")
    m._engine_lib = no_library
    m._ensure_engine = lambda device: no_library()
    return m


def test_python_argument_checks_raise_before_any_library_call():
    m = _model()
    p = torch.zeros(1, 4, 3, 16, 16)
    pos = torch.zeros(1, 4, 2)
    with pytest.raises(RuntimeError, match="MI355X only"):                      # CPU tensors: no fallback
        m.forward_rollout((p, p), (pos, pos), None)
    with pytest.raises(ValueError, match="p_ref, p_dist"):
        m.forward_rollout((p, p, p), (pos, pos, pos), None)
    m.train()
    with pytest.raises(NotImplementedError):
        m.forward_rollout((p, p), (pos, pos), None)
    m.eval()
    m._FP8_EXPERIMENT = True
    with pytest.raises(NotImplementedError, match="fp8"):
        m.forward_rollout((p, p), (pos, pos), None)
    assert Rollout._fields == ("rollout", "last_attention")
    doc = VTAMIQ.forward_rollout.__doc__
    for other in ("forward_varlen", "forward_group", "forward_cached", "forward_pairwise"):
        assert other in doc
