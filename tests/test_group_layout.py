"""forward_group / encode_reference / forward_cached without a GPU: the declarations, the exports and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from vtamiq_amd import VTAMIQ, ReferenceFeatures, StaleReferenceError, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> number of arguments
ENTRIES = {"vtq_forward_group": 13, "vtq_forward_group_tokens": 13, "vtq_encode_reference": 9, "vtq_forward_cached": 12}


@pytest.fixture(scope="module")
def lib():
    from vtamiq_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_lib_binds_and_exports_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "vtamiq_hip.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name, nargs in ENTRIES.items():
        decl = re.search(r"^int\s+" + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and _lib.SIGNATURES[name][0] is C.c_int
        assert re.search(r"\sT\s+" + name + r"$", exported, re.M), name
    assert int(re.search(r"#define\s+VTQ_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == _lib.ABI_VERSION == lib.vtq_abi_version()
    assert not any(n.startswith("vtq_k_") for n in ENTRIES)        # the kernel-contract table of test_gpu_footprint.py stays complete


def test_bad_arguments_are_refused_without_touching_a_device(lib):
    """The checks that need no device come first and name the entry; `fake` is never dereferenced."""
    fake = C.c_void_p(0x1000)
    ok = (C.c_int32 * 3)(1, 0, 1)
    err = lambda: lib.vtq_last_error()
    group = lambda fn, h, G, M, N, ix: fn(h, fake, fake, fake, fake, None, None, G, M, N, ix, fake, None)
    for fn, name in ((lib.vtq_forward_group, b"vtq_forward_group"), (lib.vtq_forward_group_tokens, b"vtq_forward_group_tokens")):
        assert group(fn, None, 2, 3, 8, ok) != 0 and name in err() and b"null handle" in err()
        assert group(fn, None, 2, 3, 8, None) != 0 and name in err() and b"ref_index" in err()
        for G, M, N, what in ((0, 3, 8, b"G=0"), (2, 0, 8, b"M=0"), (2, 3, 0, b"N=0"), (-1, 3, 8, b"G=-1")):
            assert group(fn, fake, G, M, N, ok) != 0 and name in err() and what in err()
        assert group(fn, fake, 1, 3, 8, ok) != 0 and name in err() and b"ref_index[0] = 1 outside [0, 1)" in err()
        assert group(fn, fake, 2, 3, 8, (C.c_int32 * 3)(1, 0, -1)) != 0 and b"ref_index[2] = -1" in err()
    enc = lambda h, G, N: lib.vtq_encode_reference(h, fake, 0, fake, None, G, N, fake, None)
    assert enc(None, 2, 8) != 0 and b"vtq_encode_reference" in err() and b"null handle" in err()
    assert enc(fake, 0, 8) != 0 and b"vtq_encode_reference" in err() and b"G=0" in err()
    assert enc(fake, 2, 0) != 0 and b"vtq_encode_reference" in err() and b"N=0" in err()
    cached = lambda h, G, M, N, ix: lib.vtq_forward_cached(h, fake, G, fake, 0, fake, None, M, N, ix, fake, None)
    name = b"vtq_forward_cached"
    assert cached(None, 2, 3, 8, ok) != 0 and name in err() and b"null handle" in err()
    assert cached(None, 2, 3, 8, None) != 0 and name in err() and b"ref_index" in err()
    for G, M, N, what in ((0, 3, 8, b"G=0"), (2, 0, 8, b"M=0"), (2, 3, 0, b"N=0")):
        assert cached(fake, G, M, N, ok) != 0 and name in err() and what in err()
    assert cached(fake, 1, 3, 8, ok) != 0 and name in err() and b"outside [0, 1)" in err()


def _cpu_model(**kw):
    return VTAMIQ(vit_config=dict(variant="ViT-B16", num_keep_layers=1, pretrained=False), precision="bf16", **kw).eval()


def _cpu_ref(m, G):
    return ReferenceFeatures(torch.zeros(G, m.spec.hidden_size), m.engine_precision, 0, m.engine_options, m._signature())


def test_ref_index_is_checked_on_the_host_before_any_device_work():
    """The Python entries check `ref_index` before they look at a device: CPU tensors get that far, and only a well-formed call meets the
    next refusal, forward()'s own (no CPU path)."""
    m = _cpu_model()
    G, M = 2, 3
    pr, pd = torch.zeros(G, 8, 3, 16, 16), torch.zeros(M, 8, 3, 16, 16)
    qr, qd = torch.zeros(G, 8, 2), torch.zeros(M, 8, 2)
    ref = _cpu_ref(m, G)
    calls = (lambda ix: m.forward_group((pr, pd), (qr, qd), (None, None), ix), lambda ix: m.forward_cached(ref, pd, qd, None, ix))
    for call in calls:
        for bad in ([0, 1], [0, 1, 1, 0], [0, 1, 2], [0, -1, 1], [0, 1.0, 1], [0, 0.5, 1], [0, True, 1], ["0", 1, 1], torch.tensor([0.0, 1.0, 1.0]),
                    torch.tensor([[0, 1, 1]]), torch.tensor([True, False, True]), None):
            with pytest.raises(ValueError, match="ref_index"):
                call(bad)
        for good in ([1, 0, 1], (0, 0, 0), [1, 1, 1], torch.tensor([1, 0, 1]), torch.tensor([0, 1, 0], dtype=torch.int32)):
            with pytest.raises(RuntimeError, match="MI355X"):
                call(good)
    with pytest.raises(RuntimeError, match="MI355X"):                  # None: distorted image m against reference m, G == M
        m.forward_cached(_cpu_ref(m, M), pd, qd, None)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.forward_group((pd, pd), (qd, qd), (None, None), None)
    if torch.cuda.is_available():                                      # (a CUDA tensor is refused for what reading it would cost)
        with pytest.raises(ValueError, match="CUDA"):
            calls[0](torch.tensor([1, 0, 1], device="cuda"))


def test_cuda_ref_index_is_refused_by_its_device_type():
    """Without a GPU: a tensor that merely reports a non-CPU device is refused before anything reads it."""
    m = _cpu_model()
    meta = torch.empty(3, dtype=torch.int64, device="meta")
    pd, qd = torch.zeros(3, 8, 3, 16, 16), torch.zeros(3, 8, 2)
    with pytest.raises(ValueError, match="CUDA"):
        m.forward_group((torch.zeros(2, 8, 3, 16, 16), pd), (torch.zeros(2, 8, 2), qd), (None, None), meta)
    with pytest.raises(ValueError, match="CUDA"):
        m.forward_cached(_cpu_ref(m, 2), pd, qd, None, meta)


def test_stale_references_are_refused_on_the_host():
    m = _cpu_model()
    pd, qd = torch.zeros(3, 8, 3, 16, 16), torch.zeros(3, 8, 2)
    ref = _cpu_ref(m, 2)
    for attr, value in (("precision", "fp16x3"), ("engine_options", _lib.OPT_FULL_LAST_LAYER)):
        old = getattr(m, attr)
        setattr(m, attr, value)
        with pytest.raises(StaleReferenceError):
            m.forward_cached(ref, pd, qd, None, [0, 1, 1])
        setattr(m, attr, old)
    with pytest.raises(StaleReferenceError):
        _cpu_model().forward_cached(ref, pd, qd, None, [0, 1, 1])      # another model
    m.load_state_dict(m.state_dict())
    with pytest.raises(ValueError):
        m.forward_cached(ref, pd, qd, None, [0, 1, 1])
    assert issubclass(StaleReferenceError, ValueError)
    with pytest.raises(TypeError):
        m.forward_cached(torch.zeros(2, 768), pd, qd, None, [0, 1, 1])


def test_train_mode_and_the_fp8_model_are_refused():
    m = _cpu_model().train()
    pr, pd = torch.zeros(2, 8, 3, 16, 16), torch.zeros(3, 8, 3, 16, 16)
    qr, qd = torch.zeros(2, 8, 2), torch.zeros(3, 8, 2)
    ref = _cpu_ref(m, 2)
    for call in (lambda k: k.forward_group((pr, pd), (qr, qd), (None, None), [0, 1, 1]), lambda k: k.encode_reference(pr, qr),
                 lambda k: k.forward_cached(ref, pd, qd, None, [0, 1, 1])):
        with pytest.raises(NotImplementedError, match="eval"):
            call(m)
    from vtamiq_amd.experimental_fp8 import VTAMIQFp8
    f8 = VTAMIQFp8(vit_config=dict(variant="ViT-B16", num_keep_layers=1, pretrained=False)).eval()
    for call in (lambda k: k.forward_group((pr, pd), (qr, qd), (None, None), [0, 1, 1]), lambda k: k.encode_reference(pr, qr),
                 lambda k: k.forward_cached(ref, pd, qd, None, [0, 1, 1])):
        with pytest.raises(NotImplementedError, match="fp8"):
            call(f8)
