"""vtq_forward_varlen / vtq_vl_attention without a GPU: the declarations, the host-built attention block table and the refusals."""
import ctypes as C
import os
import re

import pytest

from vtamiq_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vtq_forward_varlen", "vtq_vl_attention", "vtq_vl_attention_blocks"]
LENGTHS = [9, 64, 65, 128, 129, 257, 63]


@pytest.fixture(scope="module")
def lib():
    from vtamiq_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_lib_binds_the_entries(lib):
    hdr = open(os.path.join(ROOT, "include", "vtamiq_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"^int\s+" + name + r"\(", hdr, re.M), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert int(re.search(r"#define\s+VTQ_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10 == _lib.ABI_VERSION == lib.vtq_abi_version()
    assert not any(n.startswith("vtq_k_") for n in ENTRIES)        # the kernel-contract table of test_gpu_footprint.py stays complete


def _blocks(lib, lengths, H):
    n = len(lengths)
    arr = (C.c_int32 * n)(*lengths)
    count = lib.vtq_vl_attention_blocks(n, arr, H, None, 0)
    assert count > 0
    out = (C.c_int32 * (4 * count))()
    assert lib.vtq_vl_attention_blocks(n, arr, H, out, count) == count
    return [tuple(out[4 * i:4 * i + 4]) for i in range(count)]


@pytest.mark.parametrize("H", [768, 1024])
@pytest.mark.parametrize("lengths", [LENGTHS, LENGTHS[::-1]])
def test_block_table(lib, lengths, H):
    """Every (sequence, 128-row block, head) exactly once; first rows = the prefix sums of the lengths; the blocks of one (sequence, head)
    are consecutive work ids (the kernel keeps consecutive ids on one XCD, where they share K / V)."""
    tab = _blocks(lib, lengths, H)
    nh = H // 64
    prefix = [sum(lengths[:j]) for j in range(len(lengths))]
    want = {(prefix[j], lengths[j], qb, h) for j in range(len(lengths)) for qb in range((lengths[j] + 127) // 128) for h in range(nh)}
    assert len(tab) == len(want) == nh * sum((s + 127) // 128 for s in lengths)
    assert set(tab) == want                                            # exactly once each: equal sizes, equal sets
    # contiguity: the work ids of one (first row, head) form one run, in block order
    runs = {}
    for w, (row0, S, qb, h) in enumerate(tab):
        runs.setdefault((row0, h), []).append((w, qb))
    for (row0, h), r in runs.items():
        ids = [w for w, _ in r]
        assert ids == list(range(ids[0], ids[0] + len(r))), (row0, h)
        assert [qb for _, qb in r] == list(range(len(r)))
    # a short cap writes only that many entries
    n = len(lengths)
    out = (C.c_int32 * 8)(*([-7] * 8))
    assert lib.vtq_vl_attention_blocks(n, (C.c_int32 * n)(*lengths), H, out, 1) == len(tab)
    assert tuple(out[:4]) == tab[0] and list(out[4:]) == [-7] * 4


def test_bad_arguments_are_refused_without_touching_a_device(lib):
    """As test_abi_rejects_bad_arguments_without_touching_a_gpu: the checks that need no device come first and name the entry."""
    one = (C.c_int32 * 1)(8)
    zero = (C.c_int32 * 2)(8, 0)
    err = lambda: lib.vtq_last_error()
    fake = C.c_void_p(0x1000)              # never dereferenced: every call below is refused on an argument checked before it
    assert lib.vtq_forward_varlen(None, fake, fake, fake, fake, None, None, 1, one, fake, None) != 0
    assert b"vtq_forward_varlen" in err() and b"null handle" in err()
    assert lib.vtq_forward_varlen(None, fake, fake, fake, fake, None, None, 1, None, fake, None) != 0
    assert b"vtq_forward_varlen" in err() and b"n_patches" in err()
    assert lib.vtq_forward_varlen(None, fake, fake, fake, fake, None, None, 0, one, fake, None) != 0
    assert b"vtq_forward_varlen" in err() and b"B=0" in err()
    assert lib.vtq_forward_varlen(None, fake, fake, fake, fake, None, None, 2, zero, fake, None) != 0
    assert b"vtq_forward_varlen" in err() and b"n_patches[1] = 0" in err()
    assert lib.vtq_vl_attention_blocks(0, one, 768, None, 0) == -1
    assert lib.vtq_vl_attention_blocks(1, None, 768, None, 0) == -1
    assert lib.vtq_vl_attention_blocks(2, zero, 768, None, 0) == -1
    assert lib.vtq_vl_attention_blocks(1, one, 100, None, 0) == -1
    assert lib.vtq_vl_attention(fake, 0, fake, 0, 1, None, 768, 19, None) != 0
    assert b"vtq_vl_attention" in err() and b"null" in err()
    assert lib.vtq_vl_attention(fake, 0, fake, 0, 0, one, 768, 19, None) != 0 and b"vtq_vl_attention" in err()
    assert lib.vtq_vl_attention(fake, 0, fake, 0, 2, zero, 768, 19, None) != 0 and b"vtq_vl_attention" in err()
    assert lib.vtq_vl_attention(fake, 0, fake, 0, 1, one, 768, 18, None) != 0 and b"format" in err()      # no 2-term attention


def test_forward_varlen_refuses_bad_lengths_on_the_host():
    """The Python entry checks `lengths` before it looks at a tensor or a device."""
    import torch
    from vtamiq_amd import VTAMIQ
    m = VTAMIQ(vit_config=dict(variant="ViT-B16", num_keep_layers=1, pretrained=False), precision="bf16").eval()
    p = torch.zeros(8, 3, 16, 16)
    pos = torch.zeros(8, 2)
    for bad in ([], [8, 0], [4, -4, 8], torch.tensor([4.0, 4.0])):
        with pytest.raises(ValueError, match="lengths"):
            m.forward_varlen((p, p), (pos, pos), (None, None), bad)
    no = "not a tensor"                                                # integers only, as every other lengths=; checked before a tensor is looked at
    for bad in ([4.0, 4.0], [True, 7]):
        with pytest.raises(ValueError, match="lengths"):
            m.forward_varlen((no, no), (no, no), (None, None), bad)
    with pytest.raises(ValueError, match="sum\\(lengths\\)"):
        m.forward_varlen((p, p), (pos, pos), (None, None), [3, 4])
    with pytest.raises(RuntimeError, match="MI355X"):                  # well-formed: the next refusal is forward()'s own (CPU tensors)
        m.forward_varlen((p, p), (pos, pos), (None, None), torch.tensor([3, 5]))
