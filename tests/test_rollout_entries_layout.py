"""The rollout forms of the variable-length, group and cached entries without a GPU: every new entry is declared, exported and bound with
matching argument counts, the headers state the exact extents, DESIGN.md names the new kernels, the Python argument checks come before any
library call, and the C entries refuse a bad batch description on a NULL handle with text that names the entry and the argument."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

from vtamiq_amd import VTAMIQ, ReferenceFeatures, Rollout, _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> (its base entry, arguments)
ENTRIES = {
    "vtq_forward_varlen_rollout": ("vtq_forward_varlen", 13),
    "vtq_forward_group_rollout": ("vtq_forward_group", 15),
    "vtq_forward_group_rollout_tokens": ("vtq_forward_group_tokens", 15),
    "vtq_encode_reference_rollout": ("vtq_encode_reference", 11),
    "vtq_forward_cached_rollout": ("vtq_forward_cached", 14),
    "vtq_forward_group_varlen_rollout": ("vtq_forward_group_varlen", 16),
    "vtq_encode_reference_varlen_rollout": ("vtq_encode_reference_varlen", 10),
    "vtq_forward_cached_varlen_rollout": ("vtq_forward_cached_varlen", 13),
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def _declared(hdr, name):
    m = re.search(r"^int\s+" + name + r"\(([^;]*?)\);", hdr, re.M | re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


def test_entries_are_declared_exported_and_bound(lib):
    hdr = _read("include", "vtamiq_hip.h")
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name, (base, nargs) in ENTRIES.items():
        args = _declared(hdr, name)
        sig = _lib.SIGNATURES[name]
        assert len(args) == nargs == len(sig[1]) and sig[0] is C.c_int, name
        assert re.search(r"\bT " + name + r"$", exported, re.M), name
        assert getattr(lib, name).argtypes == sig[1], name
        # the base entry's arguments with the two outputs in front of the stream
        assert args[-3:] == ["float* rollout_out", "float* last_attention_out", "void* stream"], name
        assert args[:-3] + args[-1:] == _declared(hdr, base), name
        base_sig = _lib.SIGNATURES[base][1]
        assert sig[1] == base_sig[:-1] + [C.c_void_p, C.c_void_p] + base_sig[-1:], name
    assert "vtq_forward_pairwise_rollout" not in hdr and not hasattr(lib, "vtq_forward_pairwise_rollout")
    unit = _read("include", "vtamiq_hip_rollout.h")
    decl = re.search(r"\bvtq_vl_rollout_step\s*\(([^;]*?)\)\s*;", unit, re.S)
    assert decl and len(decl.group(1).split(",")) == 11 == len(_lib.ROLLOUT_SIGNATURES["vtq_vl_rollout_step"][1])
    assert re.search(r"\bT vtq_vl_rollout_step$", exported, re.M)
    assert lib.vtq_vl_rollout_step.argtypes == _lib.ROLLOUT_SIGNATURES["vtq_vl_rollout_step"][1]
    assert "vtq_vl_rollout_step" not in _lib.SIGNATURES and "vtq_vl_rollout_step" not in hdr      # the vtq_k_* table of vtamiq_hip.h stays as it is
    assert int(re.search(r"#define\s+VTQ_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == _lib.ABI_VERSION == lib.vtq_abi_version()


def test_headers_state_the_exact_extents():
    hdr = _read("include", "vtamiq_hip.h")
    doc = hdr[hdr.index("rollout forms of the variable-length and one-to-many entries"):hdr.index("int  vtq_forward_varlen_rollout(")]
    for text in (r"EXACTLY \(G \+ M\) \* S floats \(\[G \+ M\]\[S\], the references first\)", r"EXACTLY \(G \+ M\) \* h \* S floats",
                 r"EXACTLY G \* S floats", r"EXACTLY G \* h \* S floats", r"EXACTLY M \* S floats", r"EXACTLY M \* h \* S floats",
                 r"EXACTLY R floats", r"EXACTLY h \* R floats", r"R = the sum of S_j over the call's sequences in call order",
                 r"all B\s+\*?\s*reference sequences, then all B distorted ones"):
        assert re.search(text, doc), text
    assert len(re.findall(r"may be NULL", doc)) >= 4
    # the passage that listed the entries without a rollout form is true again (and still matches what test_group_varlen_layout.py pins)
    assert "vtq_forward_pairwise has no rollout form" in hdr and "a ragged rollout are not offered" not in hdr
    assert re.search(r"no rollout form.*?vtq_forward_group_varlen.*?5-D patches only", hdr, re.S)
    unit = _read("include", "vtamiq_hip_rollout.h")
    doc = unit[unit.index("DIFFERENT lengths"):unit.index("int  vtq_vl_rollout_step(")]
    assert "exactly R floats each" in doc and "exactly (H / 64) * ceil(S_max / 128) * R floats" in doc
    assert "seq_len = HOST int32[nseq]" in doc


def test_design_and_docs_name_the_new_kernels_and_entries():
    design = _read("DESIGN.md")
    sec0 = design[design.index("## 0."):design.index("## 1.")]
    for k in ("rollout_step_varlen_kernel", "rollout_combine_varlen_kernel", "rollout_step_block"):
        assert k in sec0, k
    assert "attention_rollout.hip" in build.SOURCES
    src = _read("vtamiq_amd", "csrc", "attention_rollout.hip")
    assert src.count("rollout_step_block<T, NSPLIT>(") == 2, "the uniform and the table-driven kernel must call ONE body"
    assert "atomicAdd" not in src
    for doc in ("README.md", "INTEGRATION.md", "HISTORY.md"):
        assert "rollout=True" in _read(doc) or "vtq_forward_group_rollout" in _read(doc), doc
    doc = VTAMIQ.forward_rollout.__doc__
    assert "have no rollout variant" not in doc and "forward_pairwise has no rollout variant" in doc


def test_python_signatures_add_one_keyword_each():
    kwonly = lambda f: [p.name for p in inspect.signature(f).parameters.values() if p.kind is p.KEYWORD_ONLY]
    assert kwonly(VTAMIQ.forward_rollout) == ["lengths"]
    assert kwonly(VTAMIQ.forward_group) == ["lengths", "rollout"]
    assert kwonly(VTAMIQ.encode_reference) == ["lengths", "rollout"]
    assert kwonly(VTAMIQ.forward_cached) == ["lengths", "rollout"]
    for f in (VTAMIQ.forward_group, VTAMIQ.encode_reference, VTAMIQ.forward_cached):
        assert inspect.signature(f).parameters["rollout"].default is False
    assert inspect.signature(VTAMIQ.forward_rollout).parameters["lengths"].default is None
    assert "rollout" not in inspect.signature(VTAMIQ.forward_pairwise).parameters
    assert Rollout._fields == ("rollout", "last_attention")


def _model():
    m = VTAMIQ(vit_config=dict(variant="ViT-B16", num_keep_layers=2, pretrained=False), calibrate=False, precision="fp16x3").eval()

    def no_library():
        raise AssertionError("the library was reached")
    m._engine_lib = no_library
    m._ensure_engine = lambda device: no_library()
    return m


def _ref(m, n):
    return ReferenceFeatures(torch.zeros(n, m.spec.hidden_size), m.engine_precision, m._token(), m.engine_options, m._signature())


def _calls(m):
    """Well-formed calls of every new form on CPU tensors."""
    p8, pos8 = torch.zeros(8, 3, 16, 16), torch.zeros(8, 2)
    u, upos = torch.zeros(2, 4, 3, 16, 16), torch.zeros(2, 4, 2)
    return {
        "forward_rollout lengths": lambda: m.forward_rollout((p8, p8), (pos8, pos8), None, lengths=[3, 5]),
        "forward_group": lambda: m.forward_group((u, u), (upos, upos), None, [0, 1], rollout=True),
        "forward_group lengths": lambda: m.forward_group((p8, p8), (pos8, pos8), None, [0, 1], lengths=([3, 5], [4, 4]), rollout=True),
        "encode_reference": lambda: m.encode_reference(u, upos, rollout=True),
        "encode_reference lengths": lambda: m.encode_reference(p8, pos8, lengths=[3, 5], rollout=True),
        "forward_cached": lambda: m.forward_cached(_ref(m, 2), u, upos, ref_index=[0, 1], rollout=True),
        "forward_cached lengths": lambda: m.forward_cached(_ref(m, 2), p8, pos8, ref_index=[0, 1], lengths=[3, 5], rollout=True),
    }


def test_python_argument_checks_raise_before_any_library_call():
    m = _model()
    for name, call in _calls(m).items():
        with pytest.raises(RuntimeError, match="MI355X only"):                   # CPU tensors: no fallback
            call()
    m.train()
    for name, call in _calls(m).items():
        with pytest.raises(NotImplementedError):
            call()
    m.eval()
    m._FP8_EXPERIMENT = True
    for name, call in _calls(m).items():
        with pytest.raises(NotImplementedError, match="fp8"):
            call()
    m._FP8_EXPERIMENT = False
    p8, pos8 = torch.zeros(8, 3, 16, 16), torch.zeros(8, 2)
    no = "not a tensor"                                                          # lengths are checked before a tensor is looked at
    for bad in ([], [8, 0], [4.5, 4], torch.tensor([4.0, 4.0]), torch.tensor([4, 4], device="meta")):       # forward_varlen's own rule
        with pytest.raises(ValueError, match="lengths"):
            m.forward_rollout((no, no), (no, no), None, lengths=bad)
    for bad in ([], [8, 0], [4.0, 4.0], [True, 7], torch.tensor([4.0, 4.0]), torch.tensor([4, 4], device="meta")):
        with pytest.raises(ValueError, match="lengths"):                         # one parser of lengths= for every entry
            m.forward_rollout((no, no), (no, no), None, lengths=bad)
        with pytest.raises(ValueError, match="lengths"):
            m.encode_reference(no, no, lengths=bad, rollout=True)
        with pytest.raises(ValueError, match="lengths"):
            m.forward_cached(_ref(m, 2), no, no, ref_index=[0, 1], lengths=bad, rollout=True)
        with pytest.raises(ValueError, match="lengths"):
            m.forward_group((no, no), (no, no), None, [0, 1], lengths=(bad, [4, 4]), rollout=True)
    with pytest.raises(ValueError, match="sum\\(lengths\\)"):
        m.forward_rollout((p8, p8), (pos8, pos8), None, lengths=[3, 4])
    with pytest.raises(ValueError, match="one tensor per pair"):
        m.forward_rollout(([p8[:3]], p8), (pos8, pos8), None, lengths=[3, 5])
    with pytest.raises(ValueError, match="pre-embedded"):
        m.forward_rollout((torch.zeros(8, 768), torch.zeros(8, 768)), (pos8, pos8), None, lengths=[3, 5])
    with pytest.raises(ValueError, match="p_ref, p_dist"):
        m.forward_rollout((p8, p8, p8), (pos8, pos8, pos8), None, lengths=[3, 5])
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        m.forward_group((p8, p8), (pos8, pos8), None, [0, 2], lengths=([3, 5], [4, 4]), rollout=True)
    with pytest.raises(TypeError):                                               # keyword-only
        m.forward_rollout((p8, p8), (pos8, pos8), None, [3, 5])


def test_bad_arguments_are_refused_on_a_null_handle(lib):
    """Every call passes a NULL handle and fake tensor pointers and is refused on an argument checked before either is looked at; the last
    call of each entry is well formed and reaches the handle."""
    arr = lambda *v: (C.c_int32 * len(v))(*v)
    fake = C.c_void_p(0x1000)              # never dereferenced

    def refused(rc, entry, *words):
        err = lib.vtq_last_error()
        assert rc != 0 and entry.encode() in err, err
        for w in words:
            assert w.encode() in err, (w, err)

    def varlen(B, n, roll=fake):
        return lib.vtq_forward_varlen_rollout(None, fake, fake, fake, fake, None, None, B, n, fake, roll, None, None)
    e = "vtq_forward_varlen_rollout"
    refused(varlen(2, None), e, "null n_patches")
    refused(varlen(0, arr(8, 8)), e, "B=0")
    refused(varlen(2, arr(8, 0)), e, "n_patches[1] = 0")
    refused(varlen(2, arr(8, 8), None), e, "null rollout_out")
    refused(varlen(2, arr(8, 8)), e, "null handle")

    for e in ("vtq_forward_group_rollout", "vtq_forward_group_rollout_tokens"):
        def group(Gn, Mn, Nn, idx, roll=fake, fn=getattr(lib, e)):
            return fn(None, fake, fake, fake, fake, None, None, Gn, Mn, Nn, idx, fake, roll, None, None)
        refused(group(2, 3, 8, None), e, "null ref_index")
        refused(group(0, 3, 8, arr(0, 0, 0)), e, "G=0")
        refused(group(2, 3, 0, arr(0, 1, 1)), e, "N=0")
        refused(group(2, 3, 8, arr(0, 2, 1)), e, "ref_index[1] = 2", "[0, 2)")
        refused(group(2, 3, 8, arr(0, 1, 1), None), e, "null rollout_out")
        refused(group(2, 3, 8, arr(0, 1, 1)), e, "null handle")

    def encode(Gn, Nn, roll=fake):
        return lib.vtq_encode_reference_rollout(None, fake, 0, fake, None, Gn, Nn, fake, roll, None, None)
    e = "vtq_encode_reference_rollout"
    refused(encode(0, 8), e, "G=0")
    refused(encode(2, -1), e, "N=-1")
    refused(encode(2, 8, None), e, "null rollout_out")
    refused(encode(2, 8), e, "null handle")

    def cached(Gn, Mn, Nn, idx, roll=fake):
        return lib.vtq_forward_cached_rollout(None, fake, Gn, fake, 0, fake, None, Mn, Nn, idx, fake, roll, None, None)
    e = "vtq_forward_cached_rollout"
    refused(cached(2, 3, 8, None), e, "null ref_index")
    refused(cached(2, 0, 8, arr(0, 1, 1)), e, "M=0")
    refused(cached(2, 3, 8, arr(2, 1, 1)), e, "ref_index[0] = 2")
    refused(cached(2, 3, 8, arr(0, 1, 1), None), e, "null rollout_out")
    refused(cached(2, 3, 8, arr(0, 1, 1)), e, "null handle")

    def groupv(Gn, Mn, n_ref, n_dist, idx, roll=fake):
        return lib.vtq_forward_group_varlen_rollout(None, fake, fake, fake, fake, None, None, Gn, Mn, n_ref, n_dist, idx, fake, roll, None, None)
    e = "vtq_forward_group_varlen_rollout"
    refused(groupv(2, 3, None, arr(8, 8, 8), arr(0, 1, 1)), e, "null n_ref")
    refused(groupv(2, 3, arr(8, 8), None, arr(0, 1, 1)), e, "null n_dist")
    refused(groupv(2, 3, arr(8, 8), arr(8, 8, 8), None), e, "null ref_index")
    refused(groupv(2, -1, arr(8, 8), arr(8, 8, 8), arr(0, 1, 1)), e, "M=-1")
    refused(groupv(2, 3, arr(8, 0), arr(8, 8, 8), arr(0, 1, 1)), e, "n_ref[1] = 0")
    refused(groupv(2, 3, arr(8, 8), arr(8, 8, -5), arr(0, 1, 1)), e, "n_dist[2] = -5")
    refused(groupv(2, 3, arr(8, 8), arr(8, 8, 8), arr(0, 1, -1)), e, "ref_index[2] = -1")
    refused(groupv(2, 3, arr(8, 8), arr(8, 8, 8), arr(0, 1, 1), None), e, "null rollout_out")
    refused(groupv(2, 3, arr(8, 8), arr(8, 8, 8), arr(0, 1, 1)), e, "null handle")

    def encodev(Gn, n, roll=fake):
        return lib.vtq_encode_reference_varlen_rollout(None, fake, fake, None, Gn, n, fake, roll, None, None)
    e = "vtq_encode_reference_varlen_rollout"
    refused(encodev(2, None), e, "null n_patches")
    refused(encodev(0, arr(8, 8)), e, "G=0")
    refused(encodev(2, arr(8, 0)), e, "n_patches[1] = 0")
    refused(encodev(2, arr(8, 8), None), e, "null rollout_out")
    refused(encodev(2, arr(8, 8)), e, "null handle")

    def cachedv(Gn, Mn, n, idx, roll=fake):
        return lib.vtq_forward_cached_varlen_rollout(None, fake, Gn, fake, fake, None, Mn, n, idx, fake, roll, None, None)
    e = "vtq_forward_cached_varlen_rollout"
    refused(cachedv(2, 3, None, arr(0, 1, 1)), e, "null n_patches")
    refused(cachedv(2, 3, arr(8, 8, 8), None), e, "null ref_index")
    refused(cachedv(2, 3, arr(0, 8, 8), arr(0, 1, 1)), e, "n_patches[0] = 0")
    refused(cachedv(2, 3, arr(8, 8, 8), arr(2, 1, 1)), e, "ref_index[0] = 2")
    refused(cachedv(2, 3, arr(8, 8, 8), arr(0, 1, 1), None), e, "null rollout_out")
    refused(cachedv(2, 3, arr(8, 8, 8), arr(0, 1, 1)), e, "null handle")

    # the unit entry: refused before any device call
    def step(qkv, nseq, n, num=_lib.NUM["fp16x3"], q_log2=1):
        return lib.vtq_vl_rollout_step(qkv, 0, fake, fake, fake, nseq, n, 768, num, q_log2, None)
    e = "vtq_vl_rollout_step"
    refused(step(None, 2, arr(8, 8)), e, "null argument")
    refused(step(fake, 2, None), e, "null argument")
    refused(step(fake, 2, arr(8, 0)), e, "sequence length < 1")
    refused(step(fake, 0, arr(8, 8)), e, "nseq=0")
    refused(step(fake, 2, arr(8, 8), num=_lib.NUM["fp16x2"]), e, "operand format")
    refused(step(fake, 2, arr(8, 8), num=_lib.NUM["fp16"]), e, "q_log2")
