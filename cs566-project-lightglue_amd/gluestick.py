"""MI355X-native GlueStick point-and-line matcher: drop-in for
``gluefactory.models.matchers.gluestick.GlueStick`` in eval mode.

Same config keys (``gluestick.py:19-36``), same ``required_data_keys`` and the same module tree
(``kenc.encoder``, ``lenc.encoder``, ``gnn.layers.<i>.update.{attn, mlp}``,
``gnn.line_layers.<i>.mlp``, ``final_proj``, ``final_line_proj``, ``bin_score``,
``line_bin_score``), so a reference state dict loads with ``strict=True``.  The forward is the HIP
path of ``liblightglue_mi355x.so`` (``include/gluestick_mi355x.h``): the SuperGlue trunk's
fp16x3 GEMM / attention kernels, the endpoint encoder, the line layer (gather, two GEMMs, an
atomic-free mean per junction), ``log_double_softmax`` and the line head.  No CPU fallback: CPU
inputs raise.

Supported: ``input_dim == descriptor_dim == 256`` (else ``ValueError``), ``line_attention: False``
and ``inter_supervision: None`` (else ``NotImplementedError`` at construction), eval mode
(training raises ``NotImplementedError``).  ``skip_init`` and ``checkpointed`` are accepted and do
nothing in eval, as in the reference (its ``AttentionalGNN`` is built with ``skip=False`` whatever
``skip_init`` says, so there is never a ``scaling`` parameter).

Deliberate differences from the reference:

* ``weights``: a path to an existing file is loaded through :meth:`state_dict_from_checkpoint`
  with ``strict=False`` (``gluestick.py:107-134``); any other non-null value is ignored -- nothing
  is ever downloaded -- and the module starts from PyTorch's default init;
* with no keypoints in an image the reference sizes ``line_matching_scores1`` by ``n_kpts1``
  (``:185-187``); here it has ``n_lines1`` entries, like every other line output;
* ``lines_junc_idx*`` must lie in ``[0, n_kpts)`` (checked); the reference's line head further needs
  them below ``2 * n_lines`` because it slices the descriptors before gathering -- here the
  junction rows are gathered directly, which is the same result wherever the reference runs;
* ``loss`` returns values without a gradient.
"""
import ctypes
import os

import torch
from torch import nn

from . import _lib
from ._native import NativeModule, _ptr
from .gs_weights import GS_DEFAULT_CONF
from .lightglue import merge_conf
from .superglue import _AttentionalPropagation, _KeypointEncoder, _mlp, _nll


class _EndPtEncoder(nn.Module):  # gluestick.py:495-514
    def __init__(self, feature_dim, layers):
        super().__init__()
        self.encoder = _mlp([5] + list(layers) + [feature_dim])
        nn.init.constant_(self.encoder[-1].bias, 0.0)


class _GNNLayer(nn.Module):  # gluestick.py:562-579
    def __init__(self, feature_dim, layer_type):
        super().__init__()
        self.type = layer_type
        self.update = _AttentionalPropagation(feature_dim, 4)


class _LineLayer(nn.Module):  # gluestick.py:582-604
    def __init__(self, feature_dim):
        super().__init__()
        self.mlp = _mlp([feature_dim * 3, feature_dim * 2, feature_dim])


class _AttentionalGNN(nn.Module):  # gluestick.py:687-711
    def __init__(self, feature_dim, layer_types):
        super().__init__()
        self.layers = nn.ModuleList([_GNNLayer(feature_dim, t) for t in layer_types])
        self.line_layers = nn.ModuleList([_LineLayer(feature_dim) for _ in range(len(layer_types) // 2)])


class GlueStick(NativeModule):
    _native_prefix = "sg_gluestick"
    _native_name = "lightglue_amd.GlueStick: tensor"
    default_conf = GS_DEFAULT_CONF
    required_data_keys = ["view0", "view1", "keypoints0", "keypoints1", "descriptors0", "descriptors1",
                          "keypoint_scores0", "keypoint_scores1", "lines0", "lines1", "lines_junc_idx0",
                          "lines_junc_idx1", "line_scores0", "line_scores1"]

    def __init__(self, conf=None):
        super().__init__()
        self.conf = conf = merge_conf(self.default_conf, conf or {})
        if int(conf.descriptor_dim) != 256 or int(conf.input_dim) != int(conf.descriptor_dim):
            raise ValueError("lightglue_amd.GlueStick: input_dim and descriptor_dim must both be 256")
        if conf.line_attention:
            raise NotImplementedError("lightglue_amd.GlueStick: line_attention is not supported")
        if conf.inter_supervision is not None:
            raise NotImplementedError("lightglue_amd.GlueStick: inter_supervision is not supported")
        if len(conf.GNN_layers) > _lib.SG_MAX_LAYERS or len(conf.keypoint_encoder) > _lib.SG_MAX_KENC:
            raise ValueError("lightglue_amd.GlueStick: too many GNN / keypoint-encoder layers")
        if not 0 <= int(conf.num_line_iterations) <= _lib.SG_GLUESTICK_MAX_LINE_ITERS:
            raise ValueError("lightglue_amd.GlueStick: num_line_iterations out of range")
        for n in conf.GNN_layers:
            if n not in ("self", "cross"):
                raise ValueError(n)
        self.kenc = _KeypointEncoder(conf.descriptor_dim, conf.keypoint_encoder)
        self.lenc = _EndPtEncoder(conf.descriptor_dim, conf.keypoint_encoder)
        self.gnn = _AttentionalGNN(conf.descriptor_dim, conf.GNN_layers)
        self.final_proj = nn.Conv1d(conf.descriptor_dim, conf.descriptor_dim, kernel_size=1)
        nn.init.constant_(self.final_proj.bias, 0.0)
        nn.init.orthogonal_(self.final_proj.weight, gain=1)
        self.final_line_proj = nn.Conv1d(conf.descriptor_dim, conf.descriptor_dim, kernel_size=1)
        nn.init.constant_(self.final_line_proj.bias, 0.0)
        nn.init.orthogonal_(self.final_line_proj.weight, gain=1)
        self.register_parameter("bin_score", nn.Parameter(torch.tensor(1.0)))
        self.register_parameter("line_bin_score", nn.Parameter(torch.tensor(1.0)))
        self._native_init()
        if conf.weights and os.path.exists(str(conf.weights)):
            obj = torch.load(str(conf.weights), map_location="cpu")
            self.load_state_dict(self.state_dict_from_checkpoint(obj), strict=False)

    @staticmethod
    def state_dict_from_checkpoint(obj):
        """The reference's key rewriting (``gluestick.py:125-134``): of a training checkpoint
        ``{"model": {...}}`` keep the keys containing ``matcher.`` and strip ``matcher.`` and
        ``module.``; anything else is taken as a state dict already."""
        if "model" in obj:
            obj = {k.replace("matcher.", ""): v for k, v in obj["model"].items() if "matcher." in k}
            obj = {k.replace("module.", ""): v for k, v in obj.items()}
        return obj

    # ------------------------------------------------------------ native handle
    def _lib_config(self):
        c = self.conf
        cfg = _lib.GSConfig()
        cfg.descriptor_dim = int(c.descriptor_dim)
        cfg.n_layers = len(c.GNN_layers)
        for i, n in enumerate(c.GNN_layers):
            cfg.layer_types[i] = 0 if n == "self" else 1
        cfg.n_kenc = len(c.keypoint_encoder)
        for i, w in enumerate(c.keypoint_encoder):
            cfg.keypoint_encoder[i] = int(w)
        cfg.num_line_iterations = int(c.num_line_iterations)
        cfg.filter_threshold = float(c.filter_threshold)
        return cfg

    def _weights_signature(self):
        return tuple((id(m), n, t.data_ptr(), t._version) for m in self.modules()
                     for n, t in list(m._parameters.items()) + list(m._buffers.items()) if t is not None)

    def _create_handle(self, lib, device, h):
        cfg = self._lib_config()
        _lib.check(lib.sg_gluestick_create(ctypes.byref(cfg), device.index or 0, ctypes.byref(h)), "sg_gluestick_create")

    def _native_state(self):
        return {k: v for k, v in self.state_dict(keep_vars=True).items() if not k.endswith("num_batches_tracked")}

    # ------------------------------------------------------------ forward (gluestick.py:136-312)
    def forward(self, data: dict, return_descriptors: bool = False) -> dict:
        """``return_descriptors``: also return the GNN output (the input of the final projections)
        as ``gnn_descriptors0/1`` [B, N, D] (a check point for tests; not a reference output)."""
        for k in self.required_data_keys:
            assert k in data, f"Missing key {k} in data"
        if self.training:
            raise NotImplementedError("lightglue_amd.GlueStick: training mode is not supported (eval forward only)")
        kpts0, kpts1 = data["keypoints0"], data["keypoints1"]
        B, M, N = kpts0.shape[0], kpts0.shape[1], kpts1.shape[1]
        L0, L1 = data["lines0"].shape[1], data["lines1"].shape[1]
        dev = kpts0.device

        def empty_lines(pred):
            pred["line_log_assignment"] = torch.zeros(B, L0, L1, dtype=torch.float, device=dev)
            pred["line_matches0"] = torch.full((B, L0), -1, device=dev, dtype=torch.int64)
            pred["line_matches1"] = torch.full((B, L1), -1, device=dev, dtype=torch.int64)
            pred["line_matching_scores0"] = torch.zeros((B, L0), device=dev, dtype=torch.float32)
            pred["line_matching_scores1"] = torch.zeros((B, L1), device=dev, dtype=torch.float32)
            return pred

        if M == 0 or N == 0:  # no detected keypoints nor lines (:156-188)
            return empty_lines({
                "log_assignment": torch.zeros(B, M, N, dtype=torch.float, device=dev),
                "matches0": torch.full((B, M), -1, device=dev, dtype=torch.int64),
                "matches1": torch.full((B, N), -1, device=dev, dtype=torch.int64),
                "matching_scores0": torch.zeros((B, M), device=dev, dtype=torch.float32),
                "matching_scores1": torch.zeros((B, N), device=dev, dtype=torch.float32),
            })
        if not kpts0.is_cuda:
            raise RuntimeError("lightglue_amd.GlueStick runs on a HIP device; inputs are on the CPU")
        device = dev

        def size_of(view):  # normalize_keypoints' size / image-shape fallback (:139-148, 470-481)
            s = view.get("image_size")
            if s is not None:
                return s.to(device=device, dtype=torch.float32).contiguous(), 0, 0
            h, w = view["image"].shape[-2:]
            return None, int(w), int(h)

        s0, w0, h0 = size_of(data["view0"])
        s1, w1, h1 = size_of(data["view1"])
        lines = L0 > 0 and L1 > 0
        j0 = data["lines_junc_idx0"].to(device=device, dtype=torch.int64).contiguous()
        j1 = data["lines_junc_idx1"].to(device=device, dtype=torch.int64).contiguous()
        if lines:  # one read-back for both images; the kernels clamp whatever they are given
            bad = torch.stack([j0.min() < 0, j1.min() < 0, j0.max() >= M, j1.max() >= N]).any()
            if bool(bad):
                raise IndexError("lightglue_amd.GlueStick: lines_junc_idx0/1 must lie in [0, number of keypoints)")
            if any(i // 2 >= len(self.gnn.line_layers) for i, n in enumerate(self.conf.GNN_layers) if n == "self") \
                    and int(self.conf.num_line_iterations) > 0:
                raise IndexError("lightglue_amd.GlueStick: a self layer has no line layer "
                                 "(gnn.line_layers holds len(GNN_layers) // 2)")

        def f32(t):
            return t.to(device=device, dtype=torch.float32).contiguous()

        k0, k1 = f32(kpts0), f32(kpts1)
        d0, d1 = f32(data["descriptors0"]), f32(data["descriptors1"])
        sc0, sc1 = f32(data["keypoint_scores0"]), f32(data["keypoint_scores1"])
        ln0, ln1 = f32(data["lines0"]), f32(data["lines1"])
        ls0, ls1 = f32(data["line_scores0"]), f32(data["line_scores1"])
        lib = self._ensure_handle(device)
        nb = ctypes.c_size_t()
        _lib.check(lib.sg_gluestick_workspace_bytes(self._handle, B, M, N, L0, L1, ctypes.byref(nb)),
                   "sg_gluestick_workspace_bytes")
        ws = self._workspace_bytes(nb.value, device)
        m0 = torch.empty((B, M), dtype=torch.int64, device=device)
        m1 = torch.empty((B, N), dtype=torch.int64, device=device)
        ms0 = torch.empty((B, M), device=device)
        ms1 = torch.empty((B, N), device=device)
        la = torch.empty((B, M + 1, N + 1), device=device)
        g0 = torch.empty((B, M, 256), device=device) if return_descriptors else None
        g1 = torch.empty((B, N, 256), device=device) if return_descriptors else None
        pred = {"log_assignment": la, "matches0": m0, "matches1": m1, "matching_scores0": ms0, "matching_scores1": ms1}
        if lines:
            pred["line_log_assignment"] = torch.empty((B, L0 + 1, L1 + 1), device=device)
            pred["line_matches0"] = torch.empty((B, L0), dtype=torch.int64, device=device)
            pred["line_matches1"] = torch.empty((B, L1), dtype=torch.int64, device=device)
            pred["line_matching_scores0"] = torch.empty((B, L0), device=device)
            pred["line_matching_scores1"] = torch.empty((B, L1), device=device)
            pred["raw_line_scores"] = torch.empty((B, L0, L1), device=device)
        else:  # the reference's zeros / -1 (:286-304)
            empty_lines(pred)
            pred["raw_line_scores"] = torch.zeros(B, L0, L1, dtype=torch.float, device=device)
        lp = (lambda k: _ptr(pred[k])) if lines else (lambda k: None)
        inp = _lib.GSInputs(B, M, N, L0, L1, _ptr(k0), _ptr(k1), _ptr(d0), _ptr(d1), _ptr(sc0), _ptr(sc1), _ptr(s0),
                            _ptr(s1), w0, h0, w1, h1, _ptr(ln0), _ptr(ln1), _ptr(j0), _ptr(j1), _ptr(ls0), _ptr(ls1))
        out = _lib.GSOutputs(_ptr(m0), _ptr(m1), _ptr(ms0), _ptr(ms1), _ptr(la), _ptr(g0), _ptr(g1),
                             lp("line_log_assignment"), lp("line_matches0"), lp("line_matches1"),
                             lp("line_matching_scores0"), lp("line_matching_scores1"), lp("raw_line_scores"))
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _lib.check(lib.sg_gluestick_forward(self._handle, ctypes.byref(inp), ctypes.byref(out), _ptr(ws), nb.value, stream),
                   "sg_gluestick_forward")
        if return_descriptors:
            pred["gnn_descriptors0"], pred["gnn_descriptors1"] = g0, g1
        return pred

    # ------------------------------------------------------------ loss values (gluestick.py:371-432)
    def loss(self, pred, data):
        """The reference's loss values (no gradient): ``sub_loss`` is ``SuperGlue.loss``'s formula,
        so ``sg_nll_loss`` (mode 0) serves the point head and, on ``gt_line_*``, the line head.
        ``sinkhorn_norm`` is a torch reduction of the log assignment.  Returns ``(losses, {})``
        (the reference's metrics need its evaluation utilities)."""
        bal = float(self.conf.loss.nll_balancing)
        wgt = float(self.conf.loss.nll_weight)
        losses = {"total": 0}
        heads = []
        if not (data["keypoints0"].shape[1] == 0 or data["keypoints1"].shape[1] == 0):
            heads.append(("", self.bin_score))
        if "lines0" in data and "lines1" in data and data["lines0"].shape[1] > 0 and data["lines1"].shape[1] > 0:
            heads.append(("line_", self.line_bin_score))
        for prefix, bin_score in heads:
            la = pred[prefix + "log_assignment"].detach()
            gt = {"gt_assignment": data["gt_" + prefix + "assignment"], "gt_matches0": data["gt_" + prefix + "matches0"],
                  "gt_matches1": data["gt_" + prefix + "matches1"]}
            out = _nll(la, gt, 0, bal)
            losses[prefix + "assignment_nll"] = out[0]
            if wgt > 0:
                losses["total"] = losses["total"] + out[0] * wgt
            losses[prefix + "num_matchable"] = out[3]
            losses[prefix + "num_unmatchable"] = out[4]
            losses[prefix + "sinkhorn_norm"] = la.exp()[:, :-1].sum(2).mean(1)
            losses[prefix + "bin_score"] = bin_score.detach()[None]
        return losses, {}

    def metrics(self, pred, data):
        raise NotImplementedError
