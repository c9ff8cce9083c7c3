"""The one-to-many entries on images of different patch counts (vtq_forward_group_varlen, vtq_encode_reference_varlen,
vtq_forward_cached_varlen; `lengths=` of forward_group / encode_reference / forward_cached) without a GPU: the declarations, the exports,
the refusals that need no device and the host checks of the Python entries."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from vtamiq_amd import VTAMIQ, ReferenceFeatures, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vtq_forward_group_varlen", "vtq_encode_reference_varlen", "vtq_forward_cached_varlen"]


@pytest.fixture(scope="module")
def lib():
    from vtamiq_amd import build
    build.build(verbose=False)
    return _lib.load()


def _declared_args(hdr, name):
    """Argument count of `int name(...)` as the header declares it."""
    m = re.search(r"^int\s+" + name + r"\(([^;]*?)\);", hdr, re.M | re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_lib_exports_and_binds_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "vtamiq_hip.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"$", exported, re.M), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert _declared_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define\s+VTQ_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == _lib.ABI_VERSION == lib.vtq_abi_version()
    assert not any(n.startswith("vtq_k_") for n in ENTRIES)        # the kernel-contract table of test_gpu_footprint.py stays complete
    # the header says where it lists the entries without a rollout form that these have none either
    assert re.search(r"no rollout form.*?vtq_forward_group_varlen.*?5-D patches only", hdr, re.S)


def test_bad_arguments_are_refused_without_touching_a_device(lib):
    """The checks of the batch description need no device and come before the handle: every call below passes a NULL handle and fake tensor
    pointers, and is refused on an argument checked before either is looked at -- except the last of each entry, which reaches the handle."""
    arr = lambda *v: (C.c_int32 * len(v))(*v)
    fake = C.c_void_p(0x1000)              # never dereferenced
    err = lambda: lib.vtq_last_error()

    def group(G, M, n_ref, n_dist, idx, q=fake, h=None):
        return lib.vtq_forward_group_varlen(h, fake, fake, fake, fake, None, None, G, M, n_ref, n_dist, idx, q, None)

    def encode(G, n, rows=fake, h=None):
        return lib.vtq_encode_reference_varlen(h, fake, fake, None, G, n, rows, None)

    def cached(G, M, n, idx, q=fake, h=None):
        return lib.vtq_forward_cached_varlen(h, fake, G, fake, fake, None, M, n, idx, q, None)

    def refused(rc, entry, *words):
        assert rc != 0
        assert entry.encode() in err(), err()
        for w in words:
            assert w.encode() in err(), (w, err())

    g = "vtq_forward_group_varlen"
    refused(group(2, 3, None, arr(8, 8, 8), arr(0, 1, 1)), g, "null n_ref")
    refused(group(2, 3, arr(8, 8), None, arr(0, 1, 1)), g, "null n_dist")
    refused(group(2, 3, arr(8, 8), arr(8, 8, 8), None), g, "null ref_index")
    refused(group(0, 3, arr(8, 8), arr(8, 8, 8), arr(0, 1, 1)), g, "G=0")
    refused(group(2, 0, arr(8, 8), arr(8, 8, 8), arr(0, 1, 1)), g, "M=0")
    refused(group(2, -1, arr(8, 8), arr(8, 8, 8), arr(0, 1, 1)), g, "M=-1")
    refused(group(2, 3, arr(8, 0), arr(8, 8, 8), arr(0, 1, 1)), g, "n_ref[1] = 0")
    refused(group(2, 3, arr(8, 8), arr(8, 0, 8), arr(0, 1, 1)), g, "n_dist[1] = 0")
    refused(group(2, 3, arr(8, 8), arr(8, 8, -5), arr(0, 1, 1)), g, "n_dist[2] = -5")
    refused(group(2, 3, arr(8, 8), arr(8, 8, 8), arr(0, 1, -1)), g, "ref_index[2] = -1")
    refused(group(2, 3, arr(8, 8), arr(8, 8, 8), arr(0, 2, 1)), g, "ref_index[1] = 2", "[0, 2)")
    refused(group(2, 3, arr(8, 8), arr(8, 8, 8), arr(0, 1, 1)), g, "null handle")

    n = "vtq_encode_reference_varlen"
    refused(encode(2, None), n, "null n_patches")
    refused(encode(0, arr(8, 8)), n, "G=0")
    refused(encode(2, arr(8, 0)), n, "n_patches[1] = 0")
    refused(encode(2, arr(8, 8)), n, "null handle")

    c = "vtq_forward_cached_varlen"
    refused(cached(2, 3, None, arr(0, 1, 1)), c, "null n_patches")
    refused(cached(2, 3, arr(8, 8, 8), None), c, "null ref_index")
    refused(cached(0, 3, arr(8, 8, 8), arr(0, 0, 0)), c, "G=0")
    refused(cached(2, 0, arr(8, 8, 8), arr(0, 1, 1)), c, "M=0")
    refused(cached(2, 3, arr(0, 8, 8), arr(0, 1, 1)), c, "n_patches[0] = 0")
    refused(cached(2, 3, arr(8, 8, 8), arr(2, 1, 1)), c, "ref_index[0] = 2")
    refused(cached(2, 3, arr(8, 8, 8), arr(0, 1, 1)), c, "null handle")


@pytest.fixture(scope="module")
def model():
    return VTAMIQ(vit_config=dict(variant="ViT-B16", num_keep_layers=1, pretrained=False), precision="bf16").eval()


def _ref(m, G):
    return ReferenceFeatures(torch.zeros(G, m.spec.hidden_size), m.engine_precision, m._token(), m.engine_options, m._signature())


BAD_LENGTHS = [[], [8, 0], [4, -4], [4.0, 4.0], [True, 7], torch.tensor([4.0, 4.0]), torch.tensor([True, True]), torch.tensor([[4, 4]]),
               torch.tensor([4, 4], device="meta"), 8]


@pytest.mark.parametrize("bad", BAD_LENGTHS, ids=[str(i) for i in range(len(BAD_LENGTHS))])
def test_lengths_are_checked_on_the_host_before_any_tensor(model, bad):
    """`lengths` is checked before a tensor or a device is looked at: the tensors here are strings, which nothing may touch."""
    m = model
    no = "not a tensor"
    with pytest.raises(ValueError, match="lengths"):
        m.encode_reference(no, no, lengths=bad)
    with pytest.raises(ValueError, match="lengths"):
        m.forward_cached(_ref(m, 2), no, no, ref_index=[0, 1], lengths=bad)
    with pytest.raises(ValueError, match="lengths"):
        m.forward_group((no, no), (no, no), None, [0, 1], lengths=(bad, [4, 4]))
    with pytest.raises(ValueError, match="lengths"):
        m.forward_group((no, no), (no, no), None, [0, 1], lengths=([4, 4], bad))


def test_python_host_checks(model):
    m = model
    p8, pos8 = torch.zeros(8, 3, 16, 16), torch.zeros(8, 2)
    p12, pos12 = torch.zeros(12, 3, 16, 16), torch.zeros(12, 2)
    # lengths for one image of forward_group only, or not a pair
    for bad in (([3, 5], None), (None, [3, 5]), ([3, 5],), [3, 5, 4], torch.tensor([3, 5])):
        with pytest.raises(ValueError, match="lengths_ref, lengths_dist"):
            m.forward_group((p8, p12), (pos8, pos12), None, [0, 1, 1], lengths=bad)
    # ref_index: one entry per distorted image, inside the references -- counted by the lengths, not by the tensors
    with pytest.raises(ValueError, match="one entry per distorted image"):
        m.forward_group((p8, p12), (pos8, pos12), None, [0, 1], lengths=([3, 5], [4, 4, 4]))
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        m.forward_group((p8, p12), (pos8, pos12), None, [0, 1, 2], lengths=([3, 5], [4, 4, 4]))
    with pytest.raises(ValueError, match="one entry per distorted image"):
        m.forward_cached(_ref(m, 2), p12, pos12, ref_index=[0, 1], lengths=[4, 4, 4])
    # sums that do not match the tensors
    with pytest.raises(ValueError, match="sum\\(lengths\\)"):
        m.forward_group((p8, p12), (pos8, pos12), None, [0, 1, 1], lengths=([3, 4], [4, 4, 4]))
    with pytest.raises(ValueError, match="sum\\(lengths\\)"):
        m.forward_group((p8, p12), (pos8, pos12), None, [0, 1, 1], lengths=([3, 5], [4, 4, 5]))
    with pytest.raises(ValueError, match="sum\\(lengths\\)"):
        m.forward_group((p8, p12), (pos8, pos8), None, [0, 1, 1], lengths=([3, 5], [4, 4, 4]))       # pos_dist too short
    with pytest.raises(ValueError, match="sum\\(lengths\\)"):
        m.encode_reference(p8, pos8, lengths=[3, 4])
    with pytest.raises(ValueError, match="sum\\(lengths\\)"):
        m.forward_cached(_ref(m, 2), p12, pos12, ref_index=[0, 1, 1], lengths=[4, 4, 5])
    # lists of per-image tensors: one per image, lengths[i] rows each
    with pytest.raises(ValueError, match="one tensor per image"):
        m.encode_reference([p8[:3], p8[3:7]], pos8, lengths=[3, 5])
    with pytest.raises(ValueError, match="one tensor per image"):
        m.encode_reference([p8[:3]], pos8, lengths=[3, 5])
    # pre-embedded ragged input is not offered
    with pytest.raises(ValueError, match="pre-embedded"):
        m.encode_reference(torch.zeros(8, 768), pos8, lengths=[3, 5])
    # well-formed calls on CPU tensors: the next refusal is forward()'s own
    with pytest.raises(RuntimeError, match="MI355X"):
        m.forward_group((p8, p12), (pos8, pos12), None, torch.tensor([0, 1, 1]), lengths=(torch.tensor([3, 5]), [4, 4, 4]))
    with pytest.raises(RuntimeError, match="MI355X"):
        m.forward_group(([p8[:3], p8[3:]], p12), ([pos8[:3], pos8[3:]], pos12), (None, None), [0, 1, 1], lengths=([3, 5], [2, 9, 1]))
    with pytest.raises(RuntimeError, match="MI355X"):
        m.encode_reference(p8, pos8, lengths=[3, 5])
    with pytest.raises(RuntimeError, match="MI355X"):
        m.forward_cached(_ref(m, 2), p12, pos12, None, [1, 0, 1], lengths=torch.tensor([4, 7, 1], dtype=torch.int32))
    # existing positional calls are unchanged, and lengths is keyword-only
    with pytest.raises(TypeError):
        m.forward_group((p8, p12), (pos8, pos12), None, [0, 1, 1], ([3, 5], [4, 4, 4]))
    with pytest.raises(RuntimeError, match="MI355X"):
        m.forward_group((p8[None], p8[None]), (pos8[None], pos8[None]), None, [0])


def test_train_mode_and_the_fp8_model_are_refused():
    m = VTAMIQ(vit_config=dict(variant="ViT-B16", num_keep_layers=1, pretrained=False), precision="bf16")
    p8, pos8 = torch.zeros(8, 3, 16, 16), torch.zeros(8, 2)
    calls = [lambda: m.forward_group((p8, p8), (pos8, pos8), None, [0, 1], lengths=([3, 5], [4, 4])),
             lambda: m.encode_reference(p8, pos8, lengths=[3, 5]),
             lambda: m.forward_cached(_ref(m, 2), p8, pos8, ref_index=[0, 1], lengths=[3, 5])]
    m.train()
    for call in calls:
        with pytest.raises(NotImplementedError, match="eval"):
            call()
    m.eval()
    m._FP8_EXPERIMENT = True
    for call in calls:
        with pytest.raises(NotImplementedError, match="fp8"):
            call()
