"""Drop-in model callable for the reference's `VTAMIQ` (modules/vtamiq/vtamiq.py:26-119) on MI355X.

Same constructor kwargs, same `state_dict()` key layout, same call
    q, aux = model((p_ref, p_dist), (pos_ref, pos_dist), (sc_ref, sc_dist))      # aux is None, q: (B,) float32
but `forward` runs the hand-written gfx950 engine (libvtamiq_hip.so) through its C ABI.

The torch modules below are PARAMETER CONTAINERS only (they give the reference's key names and shapes and are what
`load_state_dict`, `.to()`, `.parameters()` and `set_freeze_state` operate on); none of them is ever called.
There is no CPU or eager fallback: a forward on CPU tensors, in train mode, or without the built library raises.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import os
import warnings
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _lib
from .spec import ModelSpec, make_spec

_PRECISIONS = _lib.PRECISIONS
# "auto" (the default of the drop-in model): run the parity mode fp16x3, read the engine's error word after every forward (one
# 4-byte D2H + stream sync: the caller's q.cpu() / loss pays the same sync a moment later) and
#   * raise IndexError for a position outside [0, 1) or a NaN scale id, as the reference's table lookups do (transformer.py:417-421, 396-400);
#   * when an operand left the fp16 range (|v| > 65504: non-finite CLS difference) switch THIS model to "bf16x3" (fp32 range,
#     same 3-MFMA split) with a warning and re-run the call -- the fp32 reference returns finite scores there (train.py:602-607),
#     so must a drop-in.  The switch is sticky: the overflow comes from the checkpoint's activation scale.
# An explicit precision keeps the forward asynchronous (bench.py, throughput runs); check_inputs() reports on demand.
DEFAULT_PRECISION = "auto"
AUTO_FIRST, AUTO_FALLBACK = "fp16x3", "bf16x3"

_TRAIN_MSG = ("the MI355X engine implements the eval/no-grad forward only (Dropout/DropPath of vtamiq.py:72-75 and "
              "channel_attention.py:26-29 are train-time stochastic; backward is out of scope): call model.eval()")
_POS_RANGE_MSG = ("pos outside [0, 1) or a NaN scale id: index out of range in the positional- / scale-embedding table "
                  "(transformer.py:417-421, 396-400)")
_COUNT = {1: ("a", "tensor"), 2: ("two", "tensors"), 3: ("three", "tensors")}      # images per item, as the shape errors word it


def _ptr(t):
    return None if t is None else t.data_ptr()


def _i32(v):
    return (C.c_int32 * len(v))(*v)


def _image_args(ts, tokens_in):
    """(patches, pos, scales) of one list of single images as the single-image entries take them; tokens_in None: the `lengths=` forms,
    which have no such flag."""
    pt, pp, ps = ts
    return (pt.data_ptr(), pp.data_ptr(), _ptr(ps)) if tokens_in is None else (pt.data_ptr(), int(tokens_in), pp.data_ptr(), _ptr(ps))


# The C entry of each Python method, by (lengths given, rollout, pre-embedded input); a form the library does not offer has no key.  (The
# single-image entries take pre-embedded input as a flag, not as an entry of its own.)
_F, _T = False, True
_ENTRIES = {
    "pairs": {(_F, _F, _F): "vtq_forward", (_F, _F, _T): "vtq_forward_tokens", (_F, _T, _F): "vtq_forward_rollout",
              (_F, _T, _T): "vtq_forward_rollout_tokens", (_T, _F, _F): "vtq_forward_varlen", (_T, _T, _F): "vtq_forward_varlen_rollout"},
    "pairwise": {(_F, _F, _F): "vtq_forward_pairwise", (_F, _F, _T): "vtq_forward_pairwise_tokens"},
    "group": {(_F, _F, _F): "vtq_forward_group", (_F, _F, _T): "vtq_forward_group_tokens", (_F, _T, _F): "vtq_forward_group_rollout",
              (_F, _T, _T): "vtq_forward_group_rollout_tokens", (_T, _F, _F): "vtq_forward_group_varlen",
              (_T, _T, _F): "vtq_forward_group_varlen_rollout"},
    "encode": {(_F, _F, _F): "vtq_encode_reference", (_F, _F, _T): "vtq_encode_reference", (_F, _T, _F): "vtq_encode_reference_rollout",
               (_F, _T, _T): "vtq_encode_reference_rollout", (_T, _F, _F): "vtq_encode_reference_varlen",
               (_T, _T, _F): "vtq_encode_reference_varlen_rollout"},
    "cached": {(_F, _F, _F): "vtq_forward_cached", (_F, _F, _T): "vtq_forward_cached", (_F, _T, _F): "vtq_forward_cached_rollout",
               (_F, _T, _T): "vtq_forward_cached_rollout", (_T, _F, _F): "vtq_forward_cached_varlen",
               (_T, _T, _F): "vtq_forward_cached_varlen_rollout"},
}


class Rollout(NamedTuple):
    """What VTAMIQ.forward_rollout returns beside the scores (index 0 = reference image, 1 = distorted image of each pair):
      rollout         (2, B, S) fp32: attention rollout of the token the score is read from, over the S = T + N tokens of each image
                      (the T = 1 + num_extra_tokens tokens first, then the N patches in input order); > 0, each row sums to 1
      last_attention  (2, B, num_heads, S) fp32: the last layer's attention row of that token, per head
    The other entries return the same two fields over the images THEY encode (see each docstring): forward_group (ref (G, S), dist (M, S)) and
    ((G, h, S), (M, h, S)); encode_reference (G, S) / (G, h, S); forward_cached (M, S) / (M, h, S).  With `lengths=` every (n, S) tensor
    becomes a list of n tensors (S_i,) and every (n, h, S) tensor a list of (h, S_i): views into one flat allocation per field."""
    rollout: torch.Tensor
    last_attention: torch.Tensor


def _ragged_maps(roll, last, lens, T: int, nh: int):
    """The packed outputs of a variable-length rollout call as per-image views, no copies: `roll` holds the images' S_i = lens[i] + T values
    back to back, `last` image i's (nh, S_i) block at nh times its offset.  Returns (list of (S_i,), list of (nh, S_i))."""
    maps, heads, o = [], [], 0
    for n in lens:
        S = n + T
        maps.append(roll[o:o + S])
        heads.append(last[nh * o:nh * (o + S)].view(nh, S))
        o += S
    return maps, heads


class StaleReferenceError(ValueError):
    """A ReferenceFeatures object does not belong to the model state it is used with (precision, consumed token, engine options, weights):
    its rows would be scored against sequences encoded differently.  Re-encode the references."""


class ReferenceFeatures:
    """What VTAMIQ.encode_reference keeps of G reference images, for VTAMIQ.forward_cached.
      rows            (G, H) fp32: per image the consumed token's residual-stream row after the last layer, before encoder_norm.  An ordinary
                      tensor of the caller's allocator: it outlives every later forward and any growth of the engine's workspace
      precision       the engine's numerics mode that made the rows ("auto" resolved: "fp16x3" | "bf16x3")
      token           the resolved index of the consumed token (VTAMIQ.token_num; 0 = CLS)
      engine_options  the model's engine_options
      signature       the model's weight signature (VTAMIQ._signature()) at encode time
    The last four are what the rows are valid for; forward_cached raises StaleReferenceError when any of them has changed."""
    __slots__ = ("rows", "precision", "token", "engine_options", "signature")

    def __init__(self, rows, precision, token, engine_options, signature):
        self.rows, self.precision, self.token, self.engine_options, self.signature = rows, precision, int(token), int(engine_options), signature

    def __len__(self):
        return int(self.rows.shape[0])

    @staticmethod
    def cat(refs):
        """The references of several encode_reference calls as one object (rows concatenated in order); they must share what made them."""
        refs = list(refs)
        first = refs[0]
        for r in refs[1:]:
            if (r.precision, r.token, r.engine_options, r.signature) != (first.precision, first.token, first.engine_options, first.signature):
                raise StaleReferenceError("ReferenceFeatures.cat: the references were encoded under different precisions, tokens, options or weights")
        return ReferenceFeatures(torch.cat([r.rows for r in refs], 0), first.precision, first.token, first.engine_options, first.signature)


def _ref_index(ref_index, G: int, M: int):
    """`ref_index` of forward_group / forward_cached as a list of M ints in [0, G), checked on the host before any device work.  None: range(M),
    which needs G == M."""
    if ref_index is None:
        if G != M:
            raise ValueError(f"ref_index=None pairs distorted image m with reference m and needs as many references as distorted images, got G={G}, M={M}")
        return list(range(M))
    if isinstance(ref_index, torch.Tensor):
        if ref_index.device.type != "cpu":
            raise ValueError("ref_index must be a sequence of ints or a CPU integer tensor: a CUDA tensor would force a device synchronisation")
        if ref_index.dtype.is_floating_point or ref_index.dtype.is_complex or ref_index.dtype == torch.bool or ref_index.dim() != 1:
            raise ValueError("ref_index must be a 1-D integer tensor")
        ref_index = ref_index.tolist()
    ref_index = list(ref_index)
    if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in ref_index):
        raise ValueError(f"ref_index must hold integers only, got {ref_index}")
    idx = [int(v) for v in ref_index]
    if len(idx) != M:
        raise ValueError(f"ref_index must hold one entry per distorted image ({M}), got {len(idx)}")
    if any(v < 0 or v >= G for v in idx):
        raise ValueError(f"ref_index must lie in [0, {G}) (the references), got {idx}")
    return idx


def _lengths(lengths, what: str):
    """Per-image patch counts of the one-to-many entries (`lengths=`) as a list of ints >= 1, checked on the host before any tensor or device
    is looked at: a sequence of ints or a 1-D CPU integer tensor."""
    if isinstance(lengths, torch.Tensor):
        if lengths.device.type != "cpu":
            raise ValueError(f"{what} must be a sequence of ints or a CPU integer tensor: a CUDA tensor would force a device synchronisation")
        if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool or lengths.dim() != 1:
            raise ValueError(f"{what} must be a 1-D integer tensor")
        lengths = lengths.tolist()
    try:
        lengths = list(lengths)
    except TypeError:
        raise ValueError(f"{what} must be a sequence of ints or a CPU integer tensor, got {lengths!r}") from None
    if not lengths or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 for v in lengths):
        raise ValueError(f"{what} must hold at least one image and only integers >= 1, got {lengths}")
    return [int(v) for v in lengths]


def _ragged(t, lens, what: str, tail, noun: str = "image"):
    """One image's tensor of a `lengths=` call -- the items' rows concatenated, (sum(lengths), *tail), or a list of per-item (n_i, *tail)
    tensors, concatenated here on their device -- as the one "batch" of sum(lengths) rows VTAMIQ._inputs checks.  None stays None.  `noun`:
    what an item is in the message (an image of the one-to-many entries, a pair of forward_varlen)."""
    if t is None:
        return None
    total = sum(lens)
    if isinstance(t, (list, tuple)):
        if len(t) != len(lens) or any(u.shape[0] != n for u, n in zip(t, lens)):
            raise ValueError(f"{what}: a list must hold one tensor per {noun} with lengths[i] rows each")
        t = torch.cat([u.reshape(u.shape[0], *tail) for u in t], 0)
    if t.shape[0] != total or t.numel() != total * math.prod(tail):
        raise ValueError(f"{what}: {tuple(t.shape)} does not hold sum(lengths) = {total} rows of shape {tuple(tail)}")
    return t.reshape(1, total, *tail)


class _Params(nn.Module):
    """A container whose forward must never run."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container of the HIP engine; call the VTAMIQ model instead")


class _Gamma(_Params):                      # LayerScale (transformer.py:235-243)
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))


class _UvPos(_Params):                      # UvPosEmbedding (transformer.py:403-415)
    def __init__(self, n, H):
        super().__init__()
        self.positional_embeddings = nn.Parameter(torch.zeros(1, n, H).normal_(std=0.02))


class _ScaleEmb(_Params):                   # ScaleEmbedding (transformer.py:385-394)
    def __init__(self, n, H):
        super().__init__()
        self.scale_embeddings = nn.Parameter(torch.zeros(1, n, H).normal_(std=0.02))


class _Embeddings(_Params):                 # Embeddings (transformer.py:458-505)
    def __init__(self, spec: ModelSpec):
        super().__init__()
        H, P = spec.hidden_size, spec.patch_size
        if spec.use_patch_embedding:
            self.patch_embeddings = nn.Conv2d(3, H, kernel_size=P, stride=P)
        self.use_patch_embedding = spec.use_patch_embedding
        self.cls_token = nn.Parameter(torch.zeros(1, 1, H).normal_(std=0.02))
        if spec.num_extra_tokens > 0:
            self.extra_tokens = nn.Parameter(torch.zeros(1, spec.num_extra_tokens, H).normal_(std=0.02))
        if spec.use_pos_embedding:
            self.positional_embeddings = _UvPos(spec.pos_grid ** 2 + 1, H)
        if spec.use_scale_embedding:
            self.scale_embeddings = _ScaleEmb(spec.num_scales + 1, H)
        self.num_tokens = spec.num_tokens
        self.use_pos_embedding = spec.use_pos_embedding
        self.use_scale_embedding = spec.use_scale_embedding


class _Attn(_Params):                       # MultiHeadSelfAttention (transformer.py:125-146)
    def __init__(self, H):
        super().__init__()
        self.query, self.key, self.value, self.out = (nn.Linear(H, H) for _ in range(4))


class _Mlp(_Params):                        # MLP (transformer.py:197-210)
    def __init__(self, H, M):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(H, M), nn.Linear(M, H)


class _Adapter(_Params):                    # Adapter (transformer.py:177-194): x + Linear(H/4 -> H)(GELU(Linear(H -> H/4)(x)))
    def __init__(self, H):
        super().__init__()
        self.adapter = nn.Sequential(nn.Linear(H, H // 4), nn.Identity(), nn.Linear(H // 4, H))


class _EncoderLayer(_Params):               # EncoderLayer (transformer.py:246-273)
    def __init__(self, spec: ModelSpec):
        super().__init__()
        H = spec.hidden_size
        self.attention_norm = nn.LayerNorm(H, eps=1e-6)
        self.ffn_norm = nn.LayerNorm(H, eps=1e-6)
        self.ffn = _Mlp(H, spec.mlp_dim)
        self.attn = _Attn(H)
        self.use_adapters = spec.num_adapters > 0
        for a in range(1, 2 * spec.num_adapters + 1):          # adapter1 / adapter2 = pair 0 (the one the forward uses), ...
            self.add_module(f"adapter{a}", _Adapter(H))
        if spec.use_layer_scale:
            self.ls1, self.ls2 = _Gamma(H), _Gamma(H)


class _Encoder(_Params):                    # Encoder (transformer.py:328-361)
    def __init__(self, spec: ModelSpec, return_layers=False, return_attention=False):
        super().__init__()
        self.return_layers = return_layers          # read by VTAMIQ.forward_vit at every call (transformer.py:340-341, 369-372)
        self.return_attention = return_attention
        self.encoder_norm = nn.LayerNorm(spec.hidden_size, eps=1e-6)
        self.layers = nn.ModuleList(_EncoderLayer(spec) for _ in range(spec.num_layers))


class _Transformer(_Params):                # VisionTransformer (transformer.py:565-626)
    def __init__(self, spec: ModelSpec, return_layers=False, return_attention=False):
        super().__init__()
        self.hidden_size = spec.hidden_size
        self.use_layer_scale = spec.use_layer_scale
        self.use_adapters = spec.num_adapters > 0
        self.embeddings = _Embeddings(spec)
        self.encoder = _Encoder(spec, return_layers, return_attention)
        for m in self.modules():            # _init_weights (transformer.py:670-678)
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)


def _ca_layer(H, hid):                      # CALayer.conv_du (channel_attention.py:53-62, 77-80); indices 1 and 4 hold params
    m = _Params()
    m.conv_du = nn.Sequential(nn.Identity(), nn.Conv1d(H, hid, 1), nn.Identity(), nn.Identity(), nn.Conv1d(hid, H, 1),
                              nn.Identity())
    return m


def _rcab(H, hid):                          # RCAB.body (channel_attention.py:41-47); indices 1, 2, 4 hold params
    m = _Params()
    m.body = nn.Sequential(nn.Identity(), nn.PReLU(), nn.Conv1d(H, H, 1), nn.Identity(), _ca_layer(H, hid))
    return m


def _residual_group(H, hid, num_rcabs):     # ResidualGroup.body (channel_attention.py:18-25)
    m = _Params()
    m.body = nn.Sequential(*[_rcab(H, hid) for _ in range(num_rcabs)], nn.Conv1d(H, H, 1))
    return m


class VTAMIQ(nn.Module):
    _FP8_EXPERIMENT = False                       # vtamiq_amd.experimental_fp8.VTAMIQFp8 sets it

    def __init__(self, vit_config=None, calibrate=True, diff_scale=True, num_rgs=4, num_rcabs=4, rg_path_drop=0.1,
                 ca_reduction=8, predictor_dropout=0., return_features=False, precision: Optional[str] = None,
                 engine_options: int = 0, **kwargs):
        super().__init__()
        self.engine_options = int(engine_options)      # vtq_config.options (_lib.OPT_*): tests and A/B measurement; 0 = product path
        for k, v in kwargs.items():         # reference only warns about unknown kwargs (vtamiq.py:49)
            warnings.warn(f"[VTAMIQ] Unused kwarg [{k}={v}]")
        vit_config = dict(vit_config or {})
        # backbone.py:25: `pretrained` defaults to True; transformer.py:621-624 then np.load()s config["vit_weights_path"]
        pretrained = bool(vit_config.get("pretrained", True))
        weights_path = vit_config.pop("vit_weights_path", None)
        self.spec = make_spec(vit_config, calibrate=calibrate, diff_scale=diff_scale, num_rgs=num_rgs,
                              num_rcabs=num_rcabs, ca_reduction=ca_reduction)
        spec = self.spec
        H = spec.hidden_size
        self.transformer = _Transformer(spec, vit_config.get("return_layers", False), vit_config.get("return_attention", False))
        self.token_num = 0                                                   # vtamiq.py:57
        self.diff_scale = _Gamma(H) if diff_scale else nn.Sequential()       # vtamiq.py:61
        if calibrate:                                                        # vtamiq.py:63-69
            self.quality_decoder = nn.Sequential(
                *[_residual_group(H, spec.ca_hidden, num_rcabs) for _ in range(num_rgs)], nn.Conv1d(H, H, 1))
        else:
            self.quality_decoder = nn.Sequential()
        self.rg_path_drop = rg_path_drop          # stochastic only in train mode, which this path rejects
        self.predictor_dropout = predictor_dropout
        self.q_predictor = nn.Sequential(nn.Identity(), nn.Linear(H, H // 4), nn.PReLU(), nn.Identity(),
                                         nn.Linear(H // 4, 1))              # vtamiq.py:71-77 (Dropout slots 0 and 3)
        self.return_features = return_features
        precision = precision or os.environ.get("VTAMIQ_PRECISION", DEFAULT_PRECISION)
        if precision == "fp8w":                 # alias used by the round-1 review for BASELINE configs[4] ("fp8 weights"): same mode
            precision = "fp8"
        if precision != "auto" and precision not in _PRECISIONS:
            raise ValueError(f"precision must be 'auto' or one of {sorted(_PRECISIONS)}, got {precision!r}")
        if precision == "fp8" and not self._FP8_EXPERIMENT:
            raise NotImplementedError("precision 'fp8' is a throughput EXPERIMENT, not a scoring mode (SROCC 0.66 - 0.84 against the fp32 scores, "
                                      "profiles/r04_fp8_study.txt), and is not part of this model class or of the shipped library: "
                                      "vtamiq_amd.experimental_fp8.VTAMIQFp8 on a library built with `python -m vtamiq_amd.build --fp8`")
        self.precision = precision
        self._auto_fallback = False             # "auto" only: an fp16 operand overflowed, the engine now runs AUTO_FALLBACK
        self._engine = None
        self._engine_device = None
        self._engine_precision = None
        self._weights_sig = None
        self._warned_grad = False
        # VTAMIQ_VALIDATE_INPUTS=1 (or model.validate_inputs = True): synchronise after every forward and raise IndexError when a
        # position lay outside [0, 1), as the reference's table lookup does (transformer.py:417-421).  Off by default: the
        # forward stays asynchronous and such an index is clamped into the table (never read out of bounds); check_inputs()
        # reports it on demand.
        self.validate_inputs = os.environ.get("VTAMIQ_VALIDATE_INPUTS", "0") == "1"
        if pretrained:
            from .weights import default_vit_weights_path, load_vit_npz
            path = weights_path or os.environ.get("VTAMIQ_VIT_WEIGHTS") or default_vit_weights_path(self.spec.variant)
            if os.path.exists(path):
                print("ViT: Loading pretrained transformer from path:", path)          # transformer.py:623
                load_vit_npz(self, path)
            elif os.environ.get("VTAMIQ_ALLOW_MISSING_WEIGHTS", "0") == "1":
                warnings.warn(f"[VTAMIQ] pretrained=True but '{path}' does not exist: the transformer keeps its random "
                              "initialisation (VTAMIQ_ALLOW_MISSING_WEIGHTS=1)")
            else:                                  # np.load in the reference (transformer.py:622-624)
                raise FileNotFoundError(
                    f"[VTAMIQ] pretrained=True but the ViT checkpoint '{path}' does not exist.  Pass vit_config['vit_weights_path'], "
                    "set VTAMIQ_VIT_WEIGHTS, or vit_config['pretrained']=False when a full checkpoint is loaded afterwards "
                    "(VTAMIQ_ALLOW_MISSING_WEIGHTS=1 keeps the random initialisation with a warning)")

    # ---- reference surface --------------------------------------------------------------------------------
    @property
    def vit_hidden_size(self):                    # backbone.py:9-11
        return self.transformer.hidden_size

    @property
    def vit_num_layers(self):                     # backbone.py:13-15
        return len(self.transformer.encoder.layers)

    def set_freeze_state(self, freeze_state, freeze_dict):
        """requires_grad bookkeeping of vtamiq.py:81-92 / backbone.py:62-106 (host-side only; the engine never trains)."""
        requires_grad = not freeze_state
        fd = freeze_dict["freeze_dict_vit"]
        freeze_all = fd is None
        tr = self.transformer

        def set_grad(m, flag):
            for p in m.parameters():
                p.requires_grad = flag

        if freeze_all or fd["freeze_encoder"]:
            set_grad(tr.encoder, requires_grad)
            if not freeze_all and not fd["freeze_encoder_layerscale"] and tr.use_layer_scale:
                for layer in tr.encoder.layers:
                    set_grad(layer.ls1, True)
                    set_grad(layer.ls2, True)
        if freeze_all or fd["freeze_embeddings_cls_token"]:
            tr.embeddings.cls_token.requires_grad = requires_grad
        if (freeze_all or fd["freeze_embeddings_extra_tokens"]) and hasattr(tr.embeddings, "extra_tokens"):
            tr.embeddings.extra_tokens.requires_grad = requires_grad
        if (freeze_all or fd["freeze_embeddings_patch"]) and tr.embeddings.use_patch_embedding:
            set_grad(tr.embeddings.patch_embeddings, requires_grad)
        if (freeze_all or fd["freeze_embeddings_pos"]) and tr.embeddings.use_pos_embedding:
            set_grad(tr.embeddings.positional_embeddings, requires_grad)
        if (freeze_all or fd["freeze_embeddings_scale"]) and tr.embeddings.use_scale_embedding:
            set_grad(tr.embeddings.scale_embeddings, requires_grad)
        if freeze_dict["freeze_quality_decoder"]:
            set_grad(self.quality_decoder, requires_grad)
        if freeze_dict["freeze_q_predictor"]:
            set_grad(self.q_predictor, requires_grad)

    # ---- engine management --------------------------------------------------------------------------------
    def _engine_lib(self):
        """The C-ABI library this model's engine lives in: the product library (the fp8 experiment's subclass returns its own build)."""
        return _lib.load()

    def _check(self, rc: int) -> None:
        _lib.check(rc, self._engine_lib())

    def _walk(self):
        """The model's own tree as (module, name, parameter) and (parent, name, child) triples -- what _signature re-checks by identity
        on every forward.  No process-global torch hook is involved: other modules in the process cost nothing and
        change nothing here."""
        params, mods = [], []
        for mod in self.modules():
            for name, p in mod._parameters.items():
                if p is not None:
                    params.append((mod, name, p))
            for name, child in mod._modules.items():
                if child is not None:
                    mods.append((mod, name, child))
        return params, mods

    def _signature(self):
        """What the packed engine weights were made from: identity, storage and version of every parameter.  The cached walk of the
        module tree is re-validated by identity every forward (each parent still holds the same child module, each module the same
        Parameter object: ~350 `is` checks) -- which sees parameter or module REPLACEMENT and load_state_dict(assign=True) anywhere in
        THIS model's tree -- and re-done only when that fails; the rest is (data_ptr, _version) of the cached parameters, which sees
        `p.data = new_tensor` (new storage) and every in-place write that bumps the version counter (load_state_dict, optimizers).
        Not seen: in-place edits through `.data` (p.data.copy_()) -- refresh_weights()."""
        cache = self.__dict__.get("_param_cache")
        if cache is not None:
            params, mods = cache
            for mod, name, p in params:
                if mod._parameters.get(name) is not p:
                    cache = None
                    break
            else:
                for parent, name, child in mods:
                    if parent._modules.get(name) is not child:
                        cache = None
                        break
        if cache is None:
            cache = self._walk()
            self.__dict__["_param_cache"] = cache
        ps = [p for _, _, p in cache[0]]
        return (tuple(map(id, ps)), tuple(p.data_ptr() for p in ps), tuple(p._version for p in ps))

    def _release_engine(self, park: bool = False):
        """Destroy the engine -- or, park=True (the numerics mode changes on the same device: "auto" probing bf16x3 and coming back), keep
        it with its packed weights under its precision, so that a batch with non-finite inputs does not cost two engine builds and two
        weight re-packs per call.  Without park, parked engines are destroyed too."""
        eng = self.__dict__.get("_engine")
        if eng is not None:
            if park:
                self.__dict__.setdefault("_parked", {})[self.__dict__.get("_engine_precision")] = (eng, self.__dict__.get("_weights_sig"))
            else:
                self._engine_lib().vtq_destroy(eng)
        if not park:
            self._destroy_parked()
        self.__dict__["_engine"] = None
        self.__dict__["_weights_sig"] = None

    def _destroy_parked(self):
        parked = self.__dict__.setdefault("_parked", {})
        for h, _ in parked.values():
            self._engine_lib().vtq_destroy(h)
        parked.clear()

    def _forget_packed_weights(self):
        self.__dict__["_weights_sig"] = None
        parked = self.__dict__.get("_parked") or {}
        for k, (h, _) in list(parked.items()):
            parked[k] = (h, None)

    def __del__(self):
        try:
            self._release_engine()
        except Exception:           # interpreter shutdown
            pass

    def refresh_weights(self):
        """Force a re-pack of the parameters into the engine on the next forward.  REQUIRED after in-place edits through
        `.data` (p.data.copy_(), p.data.normal_(), ...): those do not bump the version counter `_signature` watches, so the
        engine would keep serving the previously packed weights.  load_state_dict / .to() / optimizer-style in-place ops on
        the parameters themselves are picked up automatically; weights.load_* call this for you."""
        self._forget_packed_weights()

    def check_inputs(self):
        """Synchronise and raise IndexError if any forward since the last check saw a position outside [0, 1) or a NaN scale id, FloatingPointError
        if one produced a non-finite CLS difference (operand range overflow, fp16 modes)."""
        if self._engine is None:
            return
        flags = self._read_flags() | self.__dict__.pop("_flags_seen", 0)    # bits an earlier look of a subclass already collected (and cleared)
        if flags & 1:
            raise IndexError(_POS_RANGE_MSG)
        if flags & 4:                               # raised by the fp8 experiment's kernels only
            raise FloatingPointError("fp8 experiment: an activation exceeded e4m3's range after scaling and was clamped to +-448 -- the "
                                     "calibrated scales do not fit this data; calibrate_fp8() on a representative batch")
        if flags & 2:
            raise FloatingPointError(
                f"non-finite encoder output in precision={self.engine_precision!r}: an activation or weight left the operand format's range "
                "(fp16 modes: |v| <= 65504) or the inputs held inf / NaN; precision='bf16x3' has the fp32 range")

    @property
    def engine_precision(self) -> str:
        """The numerics mode the engine runs: `precision`, or for "auto" fp16x3 until an operand overflow switched it to bf16x3."""
        if self.precision != "auto":
            return self.precision
        return AUTO_FALLBACK if self._auto_fallback else AUTO_FIRST

    def _read_flags(self) -> int:
        flags = C.c_int32(0)
        with torch.cuda.device(self._engine_device):
            stream = torch.cuda.current_stream(self._engine_device).cuda_stream
            self._check(self._engine_lib().vtq_input_errors(self._engine, C.byref(flags), stream))
        return flags.value

    def _enqueue(self, device, launch):
        """One forward on the engine of the current numerics mode (created / re-packed on demand)."""
        lib = self._ensure_engine(device)
        # vtamiq.py:57, 107-108: `token_num` picks the token row the head consumes ("can be CLS token or extra_token"); the reference
        # reads the attribute at every forward, so does this (a value outside the model's tokens is refused by the library)
        # (Python indexing into the (B, H, T) token rows: a negative index counts from the last register token)
        t = int(self.token_num)
        self._check(lib.vtq_set_iqa_token(self._engine, t + self.spec.num_tokens if t < 0 else t))
        launch(lib)

    def _launch_checked(self, device, launch):
        """Enqueue one forward (`launch(lib)`) and apply the model's input / range policy (see DEFAULT_PRECISION)."""
        self._enqueue(device, launch)
        if self.precision == "auto":
            flags = self._read_flags()
            if flags & 2 and not self._auto_fallback:
                # Either an operand left the fp16 range (the checkpoint's activation scale: bf16x3 cures it, and the switch stays), or
                # the inputs / weights hold inf / NaN (nothing cures that).  Run the call again in bf16x3 and look.
                self._auto_fallback = True
                self._enqueue(device, launch)
                flags2 = self._read_flags()
                if flags2 & 2:
                    # still non-finite with the fp32 operand range: the DATA is non-finite, not the format too narrow.  Go back to
                    # the parity mode (one bad batch must not leave the model in bf16x3 for good) and hand the caller
                    # what the reference's fp32 forward returns for such inputs: NaN scores (train.py:602-607), loudly.
                    self._auto_fallback = False
                    warnings.warn("[VTAMIQ] non-finite scores: the inputs or weights of this call hold inf / NaN (both the fp16x3 and "
                                  "the bf16x3 forward overflowed); the model stays in precision 'fp16x3'")
                    self._enqueue(device, launch)            # the scores handed back are the parity mode's (the healthy pairs' bits included)
                    flags2 = (flags2 & 1) | (self._read_flags() & 1)
                else:
                    # the switch is sticky: the parked fp16x3 engine (packed weights + workspace) will not be used again
                    self._destroy_parked()
                    warnings.warn(f"[VTAMIQ] an activation or weight left the fp16 operand range (|v| > 65504) in precision "
                                  f"{AUTO_FIRST!r}: this model now runs {AUTO_FALLBACK!r} (fp32 operand range, the same 3-MFMA "
                                  "split; the call was repeated)")
                flags = (flags & 1) | (flags2 & 1)
            elif flags & 2:
                warnings.warn("[VTAMIQ] non-finite scores in precision 'bf16x3': the inputs or weights of this call hold inf / NaN")
            if flags & 1:
                raise IndexError(_POS_RANGE_MSG)
        elif self.validate_inputs:
            self.check_inputs()

    def _ensure_engine(self, device: torch.device):
        lib = self._engine_lib()
        if self._engine is not None and self._engine_device != device:
            self._release_engine()
        elif self._engine is not None and self._engine_precision != self.engine_precision:
            self._release_engine(park=True)
        parked = self.__dict__.get("_parked") or {}
        if self._engine is None and self.engine_precision in parked:
            h, sig = parked.pop(self.engine_precision)
            self._engine, self._engine_device, self._engine_precision = h, device, self.engine_precision
            self._weights_sig = sig
        if self._engine is None:
            s = self.spec
            cfg = _lib.VtqConfig(
                hidden_size=s.hidden_size, mlp_dim=s.mlp_dim, num_heads=s.num_heads, num_layers=s.num_layers,
                patch_dim=s.patch_dim, pos_grid=s.pos_grid, num_extra_tokens=s.num_extra_tokens,
                num_scales=s.num_scales if s.use_scale_embedding else 0, use_layer_scale=int(s.use_layer_scale),
                calibrate=int(s.calibrate), diff_scale=int(s.diff_scale), num_rgs=s.num_rgs, num_rcabs=s.num_rcabs,
                ca_hidden=s.ca_hidden, precision=_PRECISIONS[self.engine_precision], num_adapters=s.num_adapters,
                options=self.engine_options)
            h = C.c_void_p()
            self._check(lib.vtq_create(C.byref(cfg), C.byref(h)))
            self._engine, self._engine_device, self._engine_precision = h, device, self.engine_precision
            self._weights_sig = None
            self._engine_created()
        sig = self._signature()
        if sig != self._weights_sig:
            sd = self.state_dict()
            names = [k for k, _, _ in self.spec.state_layout()]
            missing = [k for k in names if k not in sd]
            if missing:
                raise RuntimeError(f"state_dict is missing {missing[:3]}...")
            if not self.spec.use_pos_embedding:
                # use_pos_embedding=False (transformer.py:497-499, 514, 539): the model has no table and the reference adds nothing to the
                # patch rows or to CLS.  The engine's embedding epilogue always adds a table row: it gets a table of zeros (x + 0 = x).
                pk = "transformer.embeddings.positional_embeddings.positional_embeddings"
                names.append(pk)
                sd[pk] = torch.zeros(1, self.spec.pos_grid ** 2 + 1, self.spec.hidden_size, device=device, dtype=torch.float32)
            if not self.spec.use_patch_embedding:
                # use_patch_embedding=False (transformer.py:473-480): no Conv2d; the engine's patch GEMM is never launched for pre-embedded input
                # (vtq_forward_tokens), its weight slots just have to be filled
                sp = self.spec
                for pk, shape in (("transformer.embeddings.patch_embeddings.weight", (sp.hidden_size, 3, sp.patch_size, sp.patch_size)),
                                  ("transformer.embeddings.patch_embeddings.bias", (sp.hidden_size,))):
                    names.append(pk)
                    sd[pk] = torch.zeros(*shape, device=device, dtype=torch.float32)
            keep = []
            descs = (_lib.VtqTensorDesc * len(names))()
            for i, k in enumerate(names):
                t = sd[k].detach()
                if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                    t = t.to(device=device, dtype=torch.float32).contiguous()
                keep.append(t)
                descs[i] = _lib.VtqTensorDesc(k.encode(), t.data_ptr(), t.numel())
            stream = torch.cuda.current_stream(device).cuda_stream
            reload_ = self._weights_sig is not None
            self._check(lib.vtq_load_weights(self._engine, descs, len(names), stream))
            self._weights_sig = sig
            self._weights_loaded(reload_)
        return lib

    def _engine_created(self):                    # hooks of the fp8 experiment's subclass (state that must follow the engine's lifetime)
        pass

    def _weights_loaded(self, reload_: bool):
        pass

    def _apply(self, fn, *a, **k):            # .to()/.cuda()/.float(): parameter storage (possibly the objects) is replaced
        self._forget_packed_weights()
        self.__dict__["_param_cache"] = None
        return super()._apply(fn, *a, **k)

    # ---- the hot path ---------------------------------------------------------------------------------------
    @staticmethod
    def _prep(t: torch.Tensor, device) -> torch.Tensor:
        if t.device != device:
            raise ValueError(f"all inputs must live on {device}, got {t.device}")
        if t.dtype != torch.float32:
            t = t.float()                     # the loader hands everything over as f32 (train.py:254-255)
        return t if t.is_contiguous() else t.contiguous()

    def _inputs(self, patches, pos, scales, warn_grad: bool = True):
        """The input checks every entry point shares, for k = len(patches) images per item (1: forward_vit, 2: (ref, dist), 3: pairwise
        triplet): the device check, the no-autograd warning, the shapes.  Returns (device, B, N, tokens_in, patches, pos, scales) with the
        three tensor lists made fp32 and contiguous; scales is k Nones when the model has no scale embedding."""
        k = len(patches)
        how, noun = _COUNT[k]
        spec, first = self.spec, patches[0]
        device = first.device
        if device.type != "cuda":
            raise RuntimeError("VTAMIQ (vtamiq_amd) runs on an MI355X only: move the model and inputs to 'cuda'. "
                               "There is no CPU fallback on the product path.")
        if warn_grad and torch.is_grad_enabled() and not self._warned_grad and any(p.requires_grad for p in self.parameters()):
            warnings.warn("vtamiq_amd.VTAMIQ.forward returns scores without an autograd graph (inference engine)")
            self._warned_grad = True

        def got(t):                               # the triplet form names the offending tensor, the others every tensor
            return tuple(t.shape) if k == 3 else " / ".join(str(tuple(u.shape)) for u in patches)
        # Embeddings.forward (transformer.py:527-535): a 5-D tensor goes through the patch convolution, anything else is taken as pre-embedded
        # (B, N, H) rows -- whatever `use_patch_embedding` says; a model built without the convolution fails on 5-D input like the reference does
        tokens_in = first.dim() != 5
        if tokens_in:
            want = (*first.shape[:2], spec.hidden_size)
            for t in patches:
                if tuple(t.shape) != want:
                    raise ValueError(f"pre-embedded input must be {how} (B,N,{spec.hidden_size}) {noun}, got {got(t)}")
        else:
            if not spec.use_patch_embedding:
                raise AttributeError("'Embeddings' object has no attribute 'patch_embeddings' (use_patch_embedding=False: pass pre-embedded (B,N,H) rows)")
            patch = (3, spec.patch_size, spec.patch_size)
            want = (*first.shape[:2], *patch) if k == 3 else tuple(first.shape)      # (the triplet form reports a wrong patch shape here too)
            for t in patches:
                if tuple(t.shape) != want:
                    raise ValueError(f"patches must be {how} (B,N,3,P,P) {noun}, got {got(t)}")
            if tuple(first.shape[2:]) != patch:
                raise ValueError(f"patch shape {tuple(first.shape[2:])} != (3,{spec.patch_size},{spec.patch_size})")
        B, N = first.shape[:2]
        if not spec.use_pos_embedding:
            # the reference never looks at `pos` then (transformer.py:539): whatever was passed, None included, has no effect.  The
            # engine's index kernel still wants coordinates: zeros (table row 1 of the all-zero table _ensure_engine installs)
            pos = (torch.zeros(B, N, 2, device=device, dtype=torch.float32),) * k
        if any(tuple(t.shape) != (B, N, 2) for t in pos):
            raise ValueError(f"pos must be {how} (B,N,2) {noun}")
        if not spec.use_scale_embedding:
            scales = (None,) * k
        elif scales is None or any(t is None for t in scales):
            raise ValueError("Model uses scale embedding but scales is passed as None.")   # transformer.py:547-548
        elif any(t.numel() != B * N for t in scales):
            raise ValueError(f"scales must be {how} (B,N) {noun}")
        with torch.cuda.device(device):
            prep = lambda ts: [None if t is None else self._prep(t, device) for t in ts]
            return device, B, N, tokens_in, prep(patches), prep(pos), prep(scales)

    def forward(self, patches, pos, scales, _trace: Optional[torch.Tensor] = None):
        self._guard()
        patches_ref, patches_dist = patches
        device, B, N, tokens_in, (pr, pd), (qr, qd), (sr, sdist) = self._inputs((patches_ref, patches_dist), pos, scales)
        with torch.cuda.device(device):
            q = torch.empty(B, device=device, dtype=torch.float32)
            stream = torch.cuda.current_stream(device).cuda_stream

            def launch(lib):
                if _trace is not None:
                    self._check(lib.vtq_set_token_trace(self._engine, _trace.data_ptr()))
                try:
                    self._check(getattr(lib, _ENTRIES["pairs"][False, False, tokens_in])(
                        self._engine, pr.data_ptr(), pd.data_ptr(), qr.data_ptr(), qd.data_ptr(), _ptr(sr), _ptr(sdist), B, N, q.data_ptr(), stream))
                finally:
                    if _trace is not None:
                        lib.vtq_set_token_trace(self._engine, None)
            self._launch_checked(device, launch)
        return q, None

    def forward_rollout(self, patches, pos, scales, *, lengths=None):
        """forward() plus, in the same call, which patches each score looked at: attention rollout (Abnar & Zuidema) of the token the score
        is read from (`token_num`), and that token's last-layer attention row per head.  With P_l the (S, S) attention matrices
        forward_vit(return_attention) reports, A_l = (I + mean over heads of P_l) / 2:
            rollout[k, b] = e_t^T A_L A_(L-1) ... A_1          last_attention[k, b, hd] = P_L[k, b, hd, t, :]
        and nothing else (no renormalisation over patches, no discarding of heads).  The engine walks it as a row vector from the last layer
        to the first on the Q / K planes the forward leaves behind; no (S, S) matrix is stored.  The score still comes from the last layer
        pruned to its one row; that layer's Q / K rows are projected in addition, for the walk alone.
          patches, pos, scales  as forward(): (ref, dist) of 5-D patches or pre-embedded (B, N, H) rows; scales (ref, dist) or None
        Returns (q, Rollout): q (B,) fp32 with the bits of forward(); Rollout.rollout (2, B, S), Rollout.last_attention (2, B, num_heads, S),
        fp32 on the input device.  A pair's values do not depend on the batch it is in.  The input / range policy ("auto", validate_inputs,
        check_inputs) is forward()'s: a position outside [0, 1) raises IndexError, an fp16 overflow switches to bf16x3 and repeats the whole call.
        The call keeps num_layers extra QKV buffers in the engine (rollout_workspace_bytes).
          lengths  None, or B integers >= 1: pairs of DIFFERENT patch counts, inputs as in forward_varlen (concatenated (sum(lengths), ...)
                   tensors or lists of per-pair tensors, 5-D patches only).  q has the bits of forward_varlen; Rollout.rollout is then
                   (ref, dist), each a list of B tensors (S_b,), S_b = T + lengths[b], and Rollout.last_attention (ref, dist) of lists of
                   (num_heads, S_b) -- views into one flat allocation per field.  Pair b's maps have the bits of forward_rollout on pair b
                   alone; equal lengths give the bits of the call without lengths.  Integers only, as forward_varlen: floats with
                   integral values and bools are refused.
        The one-to-many entries take `rollout=True` for the same maps (forward_group, encode_reference, forward_cached, with or without
        their `lengths=`); forward_varlen's maps are this call's `lengths=` form; forward_pairwise has no rollout variant."""
        self._guard("forward_rollout")
        if len(patches) != 2:
            raise ValueError("forward_rollout expects patches = (p_ref, p_dist)")
        return self._pairs("forward_rollout", patches, pos, scales, lengths, True)

    def rollout_workspace_bytes(self, B, N):
        """Bytes of engine workspace a forward_rollout call of (B pairs, N patches) holds beside workspace_bytes(B, N)."""
        return int(self._engine_lib().vtq_rollout_workspace_bytes(self._engine, B, N)) if self._engine is not None else 0

    def forward_varlen(self, patches, pos, scales, lengths):
        """forward() on B pairs with DIFFERENT patch counts in one launch sequence: pair b has lengths[b] >= 1 patches in both images.
          patches  (ref, dist): each the pairs' patches concatenated, (sum(lengths), 3, P, P) -- or a list of B per-pair (n_b, 3, P, P) tensors,
                   concatenated here on the device
          pos      (ref, dist) of (sum(lengths), 2), scales (ref, dist) of (sum(lengths),) or None as in forward(); lists likewise
          lengths  a sequence of ints or a CPU integer tensor (a CUDA tensor is refused: reading it would synchronise the stream).  Integers
                   only, as every other `lengths=`: floats with integral values and bools are refused
        Returns (q, None), q (B,) fp32: q[b] has the bits `self((ref_b, dist_b), ...)` gives for pair b alone, in every precision; equal
        lengths give the bits of forward().  The input / range policy ("auto", validate_inputs, check_inputs) is forward()'s."""
        self._guard("forward_varlen")
        return self._pairs("forward_varlen", patches, pos, scales, lengths, False)

    def _pairs(self, what, patches, pos, scales, lengths, rollout):
        """forward_varlen and forward_rollout: B (ref, dist) pairs -- with `lengths`, of lengths[b] patches each -- and their maps where asked for."""
        lens = _lengths(lengths, "lengths") if lengths is not None else None
        if lens is not None:
            for name, ts in (("patches", patches), ("pos", pos), ("scales", scales)):
                if ts is not None and len(ts) != 2:
                    raise ValueError(f"{name} must be a (ref, dist) pair")
            pos = pos if pos is not None else (None, None)
            scales = scales if scales is not None else (None, None)
            ref, dist = (self._ragged_image(what, patches[k], pos[k], scales[k], lens, "pair") for k in (0, 1))
            patches, pos, scales = zip(ref, dist)
        device, B, N, tokens_in, (pr, pd), (qr, qd), (sr, sdist) = self._inputs(tuple(patches), pos, scales)
        B = B if lens is None else len(lens)
        with torch.cuda.device(device):
            q = torch.empty(B, device=device, dtype=torch.float32)
            # (all reference sequences, then all distorted ones)
            outs, maps = self._rollout_outputs(device, lens + lens if lens is not None else 2 * B, N) if rollout else ((), None)
            args = (pr.data_ptr(), pd.data_ptr(), qr.data_ptr(), qd.data_ptr(), _ptr(sr), _ptr(sdist), B, _i32(lens) if lens is not None else N,
                    q.data_ptr(), *outs, torch.cuda.current_stream(device).cuda_stream)
            name = _ENTRIES["pairs"][lens is not None, rollout, tokens_in]
            self._launch_checked(device, lambda lib: self._check(getattr(lib, name)(self._engine, *args)))
        if maps and lens is None:
            return q, Rollout(*(m.view(2, B, *m.shape[1:]) for m in maps))
        return q, maps and Rollout(*((m[:B], m[B:]) for m in maps))

    def _guard(self, what=None):
        """Eval only -- and, where `what` names the method, not for the fp8 experiment's model (it scores pairs and triplets only)."""
        if self.training:
            raise NotImplementedError(_TRAIN_MSG)
        if what and self._FP8_EXPERIMENT:
            raise NotImplementedError(f"{what} is not available for the fp8 experiment's model")

    def _token(self) -> int:
        t = int(self.token_num)
        return t + self.spec.num_tokens if t < 0 else t

    def _ragged_image(self, what, patches, pos, scales, lens, noun="image"):
        """One image's (patches, pos, scales) of a `lengths=` call as the one-item batches _inputs takes, their row counts checked against
        sum(lengths) -- before any device is looked at."""
        P = self.spec.patch_size
        first = patches[0] if isinstance(patches, (list, tuple)) else patches
        if first.dim() != 4:
            raise ValueError(f"{what}: with lengths, patches are (sum(lengths), 3, {P}, {P}) tensors (pre-embedded input is not offered), "
                             f"got {tuple(first.shape)}")
        pt = _ragged(patches, lens, "patches", tuple(first.shape[1:]), noun)
        ps = _ragged(pos, lens, "pos", (2,), noun) if self.spec.use_pos_embedding else pos
        sc = _ragged(scales, lens, "scales", (), noun) if self.spec.use_scale_embedding else None
        return pt, ps, sc

    def _single(self, what, patches, pos, scales, lens):
        """One list of single images through _inputs: (device, n, N, tokens_in, (patches, pos, scales)), the tensors fp32 and contiguous.  With
        lens (`lengths=`) they are the concatenated tensors, n = len(lens) and tokens_in is None: those entries take 5-D patches only."""
        if lens is not None:
            patches, pos, scales = self._ragged_image(what, patches, pos, scales, lens)
        device, n, N, tokens_in, (pt,), (ps,), (sc,) = self._inputs((patches,), (pos,), (scales,))
        return (device, n, N, tokens_in, (pt, ps, sc)) if lens is None else (device, len(lens), N, None, (pt, ps, sc))

    def _rollout_outputs(self, device, lens, N):
        """The two outputs of a rollout call, allocated: ((rollout_out, last_attention_out) pointers, (maps, heads)).  lens an int: that many
        sequences of N patches, dense (n, S) and (n, h, S) tensors; lens a list (`lengths=`): per-sequence patch counts in call order, one
        flat allocation per field and _ragged_maps' views.  Either way [:k] / [k:] of both are the first k sequences' maps and the rest's."""
        T, nh = self.spec.num_tokens, self.spec.num_heads
        if isinstance(lens, int):
            roll = torch.empty(lens, N + T, device=device, dtype=torch.float32)
            last = torch.empty(lens, nh, N + T, device=device, dtype=torch.float32)
            return (roll.data_ptr(), last.data_ptr()), (roll, last)
        R = sum(lens) + len(lens) * T                   # token rows of the call's sequences
        roll = torch.empty(R, device=device, dtype=torch.float32)
        last = torch.empty(R * nh, device=device, dtype=torch.float32)
        return (roll.data_ptr(), last.data_ptr()), _ragged_maps(roll, last, lens, T, nh)

    # ---- one-to-many scoring: every reference encoded once ----------------------------------------------------------------
    def forward_group(self, patches, pos, scales, ref_index, *, lengths=None, rollout=False):
        """M distorted images over G references in ONE call, every reference encoded once: G + M sequences where forward() on the expanded
        pairs encodes 2 M.
          patches    (p_ref, p_dist): (G, N, 3, P, P) and (M, N, 3, P, P) -- or both pre-embedded, (G | M, N, H), as in forward()
          pos        (pos_ref (G, N, 2), pos_dist (M, N, 2));  scales likewise (G | M, N), or (None, None)
          ref_index  M integers in [0, G), a sequence or a CPU integer tensor (a CUDA tensor is refused: reading it would synchronise the
                     stream); any order, repeats and unused references are allowed
        Returns (q, None), q (M,) fp32: q[m] has the bits `self((p_ref[i:i+1], p_dist[m:m+1]), ...)[0]` gives, i = ref_index[m], in every
        precision and model configuration.  The input / range policy ("auto", validate_inputs, check_inputs) is forward()'s.
          lengths    None, or (lengths_ref, lengths_dist) for images of DIFFERENT patch counts: G and M integers >= 1, each a sequence or a
                     CPU integer tensor.  patches / pos / scales are then per image the concatenated tensors, (sum, 3, P, P) / (sum, 2) /
                     (sum,), or lists of per-image tensors, as in forward_varlen (5-D patches only).  A distorted image's count need not be
                     its reference's.  q[m] has the bits of encode_reference on reference i alone followed by forward_cached on image m
                     alone -- with equal counts, of `self(...)` on the pair; all counts equal give the bits of the call without lengths.
          rollout    True: returns (q, Rollout) with forward_rollout's maps of every image the call encodes, each once: Rollout.rollout =
                     (ref (G, S), dist (M, S)), Rollout.last_attention = ((G, h, S), (M, h, S)) -- views of one allocation per field; with
                     lengths, lists of (S_i,) / (h, S_i) tensors instead.  q keeps its bits; an image's maps have the bits of forward_rollout
                     on any single pair holding it (reference side for a reference, distorted side for a distorted image)."""
        self._guard("forward_group")
        if len(patches) != 2:
            raise ValueError("forward_group expects patches = (p_ref, p_dist)")
        ragged = lengths is not None
        if ragged:
            if isinstance(lengths, torch.Tensor) or len(lengths) != 2 or lengths[0] is None or lengths[1] is None:
                raise ValueError("forward_group: lengths must be (lengths_ref, lengths_dist), one entry per image of each")
            lr, ld = _lengths(lengths[0], "lengths[0]"), _lengths(lengths[1], "lengths[1]")
            G, M = len(lr), len(ld)
        else:
            G, M = int(patches[0].shape[0]), int(patches[1].shape[0])
        idx = _ref_index(ref_index, G, M)
        pos = pos if pos is not None else (None, None)
        scales = scales if scales is not None else (None, None)
        ref, dist = (patches[0], pos[0], scales[0]), (patches[1], pos[1], scales[1])
        if ragged:                                  # both images' row counts, before a device is looked at
            ref, dist = self._ragged_image("forward_group", *ref, lr), self._ragged_image("forward_group", *dist, ld)
        device, _, N, tokens_in, (pr, qr, sr) = self._single("forward_group", *ref, None)
        device_d, _, N_d, tokens_d, (pd, qd, sdist) = self._single("forward_group", *dist, None)
        if ragged and device_d != device:
            raise ValueError("forward_group: references and distorted images must live on one device")
        if not ragged and (device_d != device or N_d != N or tokens_d != tokens_in):
            raise ValueError(f"forward_group: references and distorted images must agree in device, patch count and input form, got "
                             f"{tuple(patches[0].shape)} / {tuple(patches[1].shape)}")
        with torch.cuda.device(device):
            q = torch.empty(M, device=device, dtype=torch.float32)
            outs, maps = self._rollout_outputs(device, lr + ld if ragged else G + M, N) if rollout else ((), None)
            args = (pr.data_ptr(), pd.data_ptr(), qr.data_ptr(), qd.data_ptr(), _ptr(sr), _ptr(sdist), G, M, *((_i32(lr), _i32(ld)) if ragged else (N,)),
                    _i32(idx), q.data_ptr(), *outs, torch.cuda.current_stream(device).cuda_stream)
            name = _ENTRIES["group"][ragged, bool(rollout), tokens_in]
            self._launch_checked(device, lambda lib: self._check(getattr(lib, name)(self._engine, *args)))
        return q, maps and Rollout(*((m[:G], m[G:]) for m in maps))                  # the references first

    def encode_reference(self, patches, pos, scales=None, *, lengths=None, rollout=False):
        """Encode G reference images once, for forward_cached(): (G, N, 3, P, P) patches (or pre-embedded (G, N, H)), pos (G, N, 2), scales
        (G, N) or None.  Returns a ReferenceFeatures whose `.rows` (G, H) are an ordinary tensor of the caller's.  The input / range policy is
        forward()'s; check_inputs() raises FloatingPointError for a non-finite row.
          lengths  None, or G integers >= 1 (a sequence or a CPU integer tensor): references of DIFFERENT patch counts, patches / pos / scales
                   the concatenated (sum(lengths), ...) tensors or lists of per-image tensors, as forward_group(lengths=...).  Row g has the
                   bits of encode_reference on reference g alone.
          rollout  True: returns (ReferenceFeatures, Rollout) with forward_rollout's maps of the G references: Rollout.rollout (G, S),
                   Rollout.last_attention (G, h, S); with lengths, lists of (S_g,) / (h, S_g).  The rows keep their bits; the maps have the
                   bits forward_group(rollout=True) gives for the same references."""
        self._guard("encode_reference")
        lens = _lengths(lengths, "lengths") if lengths is not None else None
        device, G, N, tokens_in, ts = self._single("encode_reference", patches, pos, scales, lens)
        with torch.cuda.device(device):
            rows = torch.empty(G, self.spec.hidden_size, device=device, dtype=torch.float32)
            outs, maps = self._rollout_outputs(device, lens if lens is not None else G, N) if rollout else ((), None)
            args = (*_image_args(ts, tokens_in), G, _i32(lens) if lens is not None else N, rows.data_ptr(), *outs,
                    torch.cuda.current_stream(device).cuda_stream)
            name = _ENTRIES["encode"][lens is not None, bool(rollout), bool(tokens_in)]
            self._launch_checked(device, lambda lib: self._check(getattr(lib, name)(self._engine, *args)))
        # read AFTER the launch: "auto" may have switched the model to bf16x3 and repeated the call -- the rows are that run's
        ref = ReferenceFeatures(rows, self.engine_precision, self._token(), self.engine_options, self._signature())
        return (ref, Rollout(*maps)) if rollout else ref

    def _stale(self, ref: ReferenceFeatures):
        now = (self.engine_precision, self._token(), self.engine_options)
        if (ref.precision, ref.token, ref.engine_options) != now:
            return f"encoded under (precision, token, engine_options) = {(ref.precision, ref.token, ref.engine_options)}, the model is now at {now}"
        if ref.signature != self._signature():
            return "the model's weights are not the ones that encoded them (another model, load_state_dict, .to(), an optimizer step)"
        return None

    def forward_cached(self, ref: ReferenceFeatures, patches_dist, pos_dist, scales_dist=None, ref_index=None, *, lengths=None, rollout=False):
        """Score M distorted images against references encoded earlier (encode_reference): M sequences are encoded, nothing of the references.
          ref           ReferenceFeatures of G references, made by THIS model in its present state (else StaleReferenceError, a ValueError)
          patches_dist  (M, N, 3, P, P) or pre-embedded (M, N, H); pos_dist (M, N, 2); scales_dist (M, N) or None.  N need not be the
                        references' N
          ref_index     as forward_group(); None = range(M), which needs G == M
        Returns (q, None) with forward_group()'s contract.  Under precision "auto" an fp16 overflow switches the model to bf16x3 as usual and
        the call then raises StaleReferenceError: the cached rows are fp16x3 rows; encode the references again.
          lengths       None, or M integers >= 1 (a sequence or a CPU integer tensor): distorted images of DIFFERENT patch counts, the
                        tensors concatenated or lists of per-image tensors, as forward_group(lengths=...).  q[m] has the bits of
                        forward_cached on image m alone against the same rows.
          rollout       True: returns (q, Rollout) with forward_rollout's maps of the M distorted images alone (the cached references are not
                        encoded here: their maps come from encode_reference(rollout=True)): Rollout.rollout (M, S), Rollout.last_attention
                        (M, h, S); with lengths, lists of (S_m,) / (h, S_m).  The bits are forward_group(rollout=True)'s distorted side."""
        self._guard("forward_cached")
        if not isinstance(ref, ReferenceFeatures):
            raise TypeError("forward_cached takes the ReferenceFeatures of encode_reference as its first argument")
        lens = _lengths(lengths, "lengths") if lengths is not None else None
        G, M = len(ref), (len(lens) if lens is not None else int(patches_dist.shape[0]))
        idx = _ref_index(ref_index, G, M)
        why = self._stale(ref)
        if why:
            raise StaleReferenceError(f"forward_cached: the reference features are stale: {why}; encode_reference again")
        device, _, N, tokens_in, ts = self._single("forward_cached", patches_dist, pos_dist, scales_dist, lens)
        rows = ref.rows
        if rows.device != device or rows.dtype != torch.float32 or tuple(rows.shape) != (G, self.spec.hidden_size) or not rows.is_contiguous():
            raise ValueError(f"forward_cached: ref.rows must be a contiguous fp32 (G, {self.spec.hidden_size}) tensor on {device}")
        with torch.cuda.device(device):
            q = torch.empty(M, device=device, dtype=torch.float32)
            outs, maps = self._rollout_outputs(device, lens if lens is not None else M, N) if rollout else ((), None)
            args = (rows.data_ptr(), G, *_image_args(ts, tokens_in), M, _i32(lens) if lens is not None else N, _i32(idx), q.data_ptr(), *outs,
                    torch.cuda.current_stream(device).cuda_stream)
            name = _ENTRIES["cached"][lens is not None, bool(rollout), bool(tokens_in)]
            self._launch_checked(device, lambda lib: self._check(getattr(lib, name)(self._engine, *args)))
        if self.engine_precision != ref.precision:
            raise StaleReferenceError(f"forward_cached: an operand left the fp16 range and the model now runs {self.engine_precision!r}; the cached "
                                      f"rows are {ref.precision!r} rows: encode_reference again")
        return q, maps and Rollout(*maps)

    def forward_pairwise(self, patches, pos, scales):
        """Pairwise items: `patches = (p_ref, p_dist1, p_dist2)` etc.  Returns (q1, q2) == what two calls
        `self((p_ref, p_dist1), ...)[0]`, `self((p_ref, p_dist2), ...)[0]` give (train.py:286-287), bit for bit, with the
        reference image encoded once: 3B sequences instead of 4B."""
        self._guard()
        if len(patches) != 3 or (self.spec.use_pos_embedding and len(pos) != 3):
            raise ValueError("forward_pairwise expects (ref, dist1, dist2) triplets")
        device, B, N, tokens_in, pt, ps, sc = self._inputs(patches, pos, scales, warn_grad=False)
        with torch.cuda.device(device):
            q = torch.empty(2 * B, device=device, dtype=torch.float32)
            arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
            stream = torch.cuda.current_stream(device).cuda_stream
            args = (arr(pt), arr(ps), arr(sc) if sc[0] is not None else None, B, N, q.data_ptr(), stream)
            self._launch_checked(device, lambda lib: self._check(getattr(lib, _ENTRIES["pairwise"][False, False, tokens_in])(self._engine, *args)))
        return q[:B], q[B:]

    def forward_vit(self, patches, patches_pos, patches_scale, tokens_only=True, adapter_num=None):
        """VisionTransformerBackbone.forward_vit (backbone.py:54-60, transformer.py:628-641, 363-378) on the HIP engine: B single images
        (5-D patches or pre-embedded (B, N, H) rows, as one image of forward()) -> (x, attn_weights, hidden_states):
          x              encoder_norm output, (B, T, H) when tokens_only else (B, S, H) with every token row; T = 1 + num_extra_tokens, S = N + T
          hidden_states  transformer.encoder.return_layers: L tensors, the residual stream after each layer (before encoder_norm; the
                         embedding output is not one of them), sliced to [:, :T] when tokens_only; else []
          attn_weights   transformer.encoder.return_attention: L (B, num_heads, S, S) softmax probabilities; else []
        All fp32 on the input device.  The flags are read at every call, so setting them after construction takes effect."""
        self._guard("forward_vit")
        if adapter_num is not None and adapter_num >= 1 and self.spec.num_adapters > 0:
            # backbone.py:55-57: None / negative selects pair 0 when the model has adapters; a model without adapters ignores the number
            # (transformer.py:277-278), as the engine does
            raise NotImplementedError(f"adapter_num={adapter_num}: the engine applies adapter pair 0 only (adapter_num None, negative or 0)")
        device, B, N, tokens_in, (pt,), (pp,), (ps,) = self._inputs((patches,), (patches_pos,), (patches_scale,))
        spec, enc = self.spec, self.transformer.encoder
        want_states, want_probs = bool(enc.return_layers), bool(enc.return_attention)
        L, T, H, nh = spec.num_layers, spec.num_tokens, spec.hidden_size, spec.num_heads
        S = N + T
        R = T if tokens_only else S
        with torch.no_grad(), torch.cuda.device(device):
            x = torch.empty(B, R, H, device=device, dtype=torch.float32)
            states = torch.empty(L, B, R, H, device=device, dtype=torch.float32) if want_states else None
            probs = torch.empty(L, B, nh, S, S, device=device, dtype=torch.float32) if want_probs else None
            stream = torch.cuda.current_stream(device).cuda_stream
            self._launch_checked(device, lambda lib: self._check(lib.vtq_forward_vit(
                self._engine, pt.data_ptr(), int(tokens_in), pp.data_ptr(), _ptr(ps), B, N, int(not tokens_only),
                x.data_ptr(), _ptr(states), _ptr(probs), stream)))
        return x, (list(probs.unbind(0)) if want_probs else []), (list(states.unbind(0)) if want_states else [])

    # ---- measurement helpers (bench.py) ---------------------------------------------------------------------
    def profile_enable(self, classes):
        mask = 0
        for c in classes:
            mask |= 1 << _lib.KERNEL_CLASSES.index(c)
        self._check(self._engine_lib().vtq_profile_enable(self._engine, mask))

    def profile_collect(self):
        n = len(_lib.KERNEL_CLASSES)
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        self._check(self._engine_lib().vtq_profile_collect(self._engine, ms, cnt))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(_lib.KERNEL_CLASSES)}

    def workspace_bytes(self, B, N):
        return int(self._engine_lib().vtq_workspace_bytes(self._engine, B, N)) if self._engine is not None else 0
