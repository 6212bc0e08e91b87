"""MI355X-native open SuperPoint: drop-in for ``gluefactory.models.extractors.superpoint_open.SuperPoint``
(reference ``superpoint_open.py:76-210``), the MIT-licensed model of the ``superpoint-open+*`` configs.

Same config keys (:77-87, plus the BaseModel keys) and the same module tree -- ``backbone`` as an
``nn.Sequential`` of ``nn.Sequential`` of ``VGGBlock`` (``conv`` / ``activation`` / ``bn``) with the
``MaxPool2d`` members at the reference's indices, ``detector`` and ``descriptor`` -- so
``list(state_dict())`` equals the reference's 84 keys and ``superpoint_v6_from_tf.pth`` loads with a
strict ``load_state_dict``.  Same ``forward(data) -> dict`` outputs (:199-207).  The forward is the
HIP path behind ``sp_open_create`` (``include/superpoint_mi355x.h``): the nonfree extractor's
convolution kernels with a per-channel affine after the ReLU (the eval BatchNorm, folded to
``(s, t)`` at load time; the fused 2x2 pool takes the window's minimum where ``s < 0``), the 1x1
heads with their BatchNorm folded into the weights, ``grid_sample(align_corners=False)`` sampling
at the pixel centres.  No CPU fallback: CPU inputs raise.

Deliberate differences from the reference:

* the trained checkpoint is a download (:89,114-115); the module starts from PyTorch's default init
  and takes weights through ``load_state_dict``;
* BatchNorm always uses its running statistics.  The reference's frozen extractor would switch to
  batch statistics under ``pipe.train()`` unless ``freeze_batch_normalization`` is set;
* top-k ties at the selection boundary keep the lower pixel index first (``torch.topk`` leaves it
  unspecified), as the nonfree module does;
* B > 1 without ``force_num_keypoints``: equal counts are stacked (the reference fails at
  ``desc.transpose`` on its list, :193-202), unequal counts raise the reference's ``stack`` error
  (:187); ``data["ragged_keypoints"]`` returns them zero-padded with ``num_keypoints``, as the
  nonfree module does;
* ``descriptor_dim`` other than 256 and ``channels`` other than ``[64, 64, 128, 128, 256]`` raise.
"""
import ctypes
from collections import OrderedDict

import torch
from torch import nn

from . import _lib
from ._native import _ptr
from .lightglue import merge_conf
from .sp_weights import SPO_DEFAULT_CONF
from .superpoint import SuperPoint as _NonfreeSuperPoint


class VGGBlock(nn.Sequential):  # superpoint_open.py:57-73
    def __init__(self, c_in, c_out, kernel_size, relu=True):
        padding = (kernel_size - 1) // 2
        super().__init__(OrderedDict([
            ("conv", nn.Conv2d(c_in, c_out, kernel_size=kernel_size, stride=1, padding=padding)),
            ("activation", nn.ReLU(inplace=True) if relu else nn.Identity()),
            ("bn", nn.BatchNorm2d(c_out, eps=0.001)),
        ]))


class SuperPoint(_NonfreeSuperPoint):
    """Shares the native handle plumbing (weights signature, workspace, padding, the stacked /
    ragged / padded output forms) with the nonfree module; the parameter tree, the handle's
    architecture and the forward are its own."""

    default_conf = SPO_DEFAULT_CONF
    required_data_keys = ["image"]
    checkpoint_url = "https://github.com/rpautrat/SuperPoint/raw/master/weights/superpoint_v6_from_tf.pth"

    def __init__(self, conf=None):
        nn.Module.__init__(self)
        self.conf = conf = merge_conf(self.default_conf, conf or {})
        if int(conf.descriptor_dim) != 256:
            raise ValueError("lightglue_amd.SuperPointOpen: descriptor_dim must be 256")
        if list(conf.channels) != [64, 64, 128, 128, 256]:
            raise ValueError("lightglue_amd.SuperPointOpen: channels must be [64, 64, 128, 128, 256]")
        if conf.max_num_keypoints is not None and int(conf.max_num_keypoints) <= 0:
            raise ValueError("lightglue_amd.SuperPointOpen: max_num_keypoints must be None or positive")
        self.stride = 2 ** (len(conf.channels) - 2)  # superpoint_open.py:93-112
        channels = [1, *conf.channels[:-1]]
        backbone = []
        for i, c in enumerate(channels[1:], 1):
            layers = [VGGBlock(channels[i - 1], c, 3), VGGBlock(c, c, 3)]
            if i < len(channels) - 1:
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            backbone.append(nn.Sequential(*layers))
        self.backbone = nn.Sequential(*backbone)
        c = conf.channels[-1]
        self.detector = nn.Sequential(VGGBlock(channels[-1], c, 3), VGGBlock(c, self.stride ** 2 + 1, 1, relu=False))
        self.descriptor = nn.Sequential(VGGBlock(channels[-1], c, 3), VGGBlock(c, conf.descriptor_dim, 1, relu=False))
        if not conf.trainable:
            for p in self.parameters():
                p.requires_grad = False
        # the modules that own tensors (the tree is fixed here): walked once, not per forward
        self._owners = [m for m in self.modules() if isinstance(m, (nn.Conv2d, nn.BatchNorm2d))]
        self._native_init()

    # ------------------------------------------------------------ native handle
    def _create_handle(self, lib, device, h):
        c = self.conf
        cfg = _lib.SPOpenConfig(int(c.descriptor_dim), int(c.nms_radius), int(c.remove_borders or 0),
                                float(c.detection_threshold))
        _lib.check(lib.sp_open_create(ctypes.byref(cfg), device.index or 0, ctypes.byref(h)), "sp_open_create")

    def _native_state(self):
        # bn.num_batches_tracked is an int64 counter the forward does not use
        return OrderedDict((n, t) for n, t in self.state_dict(keep_vars=True).items()
                           if not n.endswith("num_batches_tracked"))

    def _weights_signature(self):  # parameters and the BatchNorm running statistics
        sig = []
        for m in self._owners:
            sig += [(id(m), n, t.data_ptr(), t._version) for n, t in m._parameters.items() if t is not None]
            if m._buffers:
                sig += [(id(m), n, m._buffers[n].data_ptr(), m._buffers[n]._version) for n in ("running_mean", "running_var")]
        return tuple(sig)

    # ------------------------------------------------------------ forward (superpoint_open.py:117-207)
    def forward(self, data: dict) -> dict:
        for k in self.required_data_keys:
            assert k in data, f"Missing key {k} in data"
        c = self.conf
        image = data["image"]
        if not image.is_cuda:
            raise RuntimeError("lightglue_amd.SuperPointOpen runs on a HIP device; inputs are on the CPU")
        if image.dim() != 4 or image.shape[1] not in (1, 3):
            raise ValueError(f"image must be [B, 1 or 3, H, W], got {tuple(image.shape)}")
        device = image.device
        image = image.float().contiguous()
        B, C, H, W = image.shape
        Hc, Wc = H // 2 // 2 // 2, W // 2 // 2 // 2
        max_kps = 0 if c.max_num_keypoints is None else int(c.max_num_keypoints)  # 0: every candidate (:166)
        if c.force_num_keypoints:
            assert max_kps > 0, "force_num_keypoints needs max_num_keypoints"
        cap = max_kps if max_kps > 0 else 64 * Hc * Wc
        lib = self._ensure_handle(device)
        ws, nb = self._workspace(lib, device, B, C, H, W, cap)
        dense_desc = torch.empty((B, Hc, Wc, 256), device=device) if c.dense_outputs else None
        kpts = torch.empty((B, cap, 2), device=device)
        scores = torch.empty((B, cap), device=device)
        desc = torch.empty((B, cap, 256), device=device) if max_kps > 0 else None
        counts = torch.empty((B,), dtype=torch.int32, device=device)
        host_counts = (ctypes.c_int32 * B)()
        # borders go at the map's edges (:138-143): no image_size
        inp = _lib.SPInputs(B, C, H, W, _ptr(image), None, max_kps, 1)
        out = _lib.SPOutputs(None, _ptr(dense_desc), cap, _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(counts),
                             ctypes.cast(host_counts, ctypes.c_void_p))
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _lib.check(lib.sp_forward(self._handle, ctypes.byref(inp), ctypes.byref(out), _ptr(ws), nb, stream), "sp_forward")
        pred = self._sparse_pred(lib, data, image, kpts, scores, desc, counts, list(host_counts), max_kps, cap, ws, nb, stream)
        if c.dense_outputs:
            pred["dense_descriptors"] = dense_desc.permute(0, 3, 1, 2)  # [B, D, Hc, Wc] view of the NHWC map
        return pred
