"""MI355X-native ALIKED: drop-in for ``gluefactory.models.extractors.aliked.ALIKED`` (reference
``aliked.py:591-786``), the extractor of the ``aliked+*`` configs.

Same config keys (:592-599, plus the BaseModel keys), the four ``model_name``s of :605-642 and the
same module tree -- ``block1..4`` (``conv1/bn1/conv2/bn2/downsample``, with ``offset_conv`` /
``regular_conv`` inside the two deformable blocks), ``conv1..4``, ``score_head.{0,2,4,6}``,
``desc_head.{offset_conv.{0,2}, sf_conv, agg_weights}`` -- so ``list(state_dict())`` equals the
reference's and the ALIKED authors' checkpoints load with a strict ``load_state_dict``.  The forward
is the HIP path behind ``sp_aliked_create`` (``include/aliked_mi355x.h``): direct
convolutions with the BatchNorm folded in, the deformable convolution, the score head and the
descriptor gathers formed from the four pyramid levels (the concatenated full-resolution map is
never written), DKD on the device, the SDDH products on the matrix cores.  No CPU fallback: CPU
inputs raise.

Outputs (:777-783): ``keypoints`` [B,N,2], ``descriptors`` [B,N,dim], ``keypoint_scores``,
``score_dispersity`` [B,N], ``score_map`` [B,1,H,W].  The reference's ``_forward`` unpacks
``self.dkd(...)`` as ``keypoints, kptscores, scoredispersitys`` (:768) while ``DKD.forward`` returns
``keypoints, scoredispersitys, kptscores`` (:240): **``keypoint_scores`` carries the soft-argmax
dispersity and ``score_dispersity`` the score sampled at the refined position.**  This module
returns what the reference returns under each key (the fixtures pin it), not what the names say.
Keypoints are ``(w, h) * (k + 1) / 2`` with ``k`` DKD's position normalised by ``(w-1, h-1)``: both
conventions are the reference's.

Deliberate differences from the reference:

* ``pretrained: True`` is a download (:601,726-730); the module starts from PyTorch's default init
  and takes weights through ``load_state_dict`` (``lightglue_amd.aliked_weights`` has a recipe);
* BatchNorm always uses its running statistics (the extractor is frozen in every config);
* top-k ties at the selection boundary keep the lower pixel index first (``torch.topk`` leaves it
  unspecified);
* DKD's loop over ``image_size`` rebinds ``w, h`` (:127), so with ``image_size`` given the reference
  converts pixel indices with the *last* image's width; here the tensor's width and height are
  used, which is the same thing whenever the last image fills the tensor;
* threshold mode with B > 1: equal counts are stacked, unequal counts raise the reference's
  ``stack`` error (:778); ``data["ragged_keypoints"] = True`` returns them zero-padded with
  ``num_keypoints``, as the SuperPoint modules do;
* an image with other than 3 channels raises ``ValueError`` (the reference's first convolution
  would fail on it); ``force_num_keypoints`` outside the top-k mode raises ``ValueError`` (an
  assert in the reference, :648).
"""
import ctypes

import torch
from torch import nn

from . import _lib
from ._native import NativeModule, _ptr
from .aliked_weights import ALIKED_CFGS, ALIKED_DEFAULT_CONF
from .lightglue import merge_conf


class DeformableConv2d(nn.Module):  # aliked.py:270-305 (mask=False)
    def __init__(self, c_in, c_out):
        super().__init__()
        self.offset_conv = nn.Conv2d(c_in, 18, kernel_size=3, stride=1, padding=1, bias=True)
        self.regular_conv = nn.Conv2d(c_in, c_out, kernel_size=3, stride=1, padding=1, bias=False)


def _conv(c_in, c_out, dcn):
    return DeformableConv2d(c_in, c_out) if dcn else nn.Conv2d(c_in, c_out, 3, 1, 1, bias=False)


class ConvBlock(nn.Module):  # aliked.py:365-389
    def __init__(self, c_in, c_out, gate):
        super().__init__()
        self.gate = gate
        self.conv1 = _conv(c_in, c_out, False)
        self.bn1 = nn.BatchNorm2d(c_out)
        self.conv2 = _conv(c_out, c_out, False)
        self.bn2 = nn.BatchNorm2d(c_out)


class ResBlock(nn.Module):  # aliked.py:398-437
    def __init__(self, c_in, c_out, gate, dcn):
        super().__init__()
        self.gate = gate
        self.conv1 = _conv(c_in, c_out, dcn)
        self.bn1 = nn.BatchNorm2d(c_out)
        self.conv2 = _conv(c_out, c_out, dcn)
        self.bn2 = nn.BatchNorm2d(c_out)
        self.downsample = nn.Conv2d(c_in, c_out, 1)


class SDDH(nn.Module):  # aliked.py:458-511 (conv2D=False, mask=False)
    def __init__(self, dims, kernel_size, n_pos, gate):
        super().__init__()
        self.offset_conv = nn.Sequential(nn.Conv2d(dims, 2 * n_pos, kernel_size=kernel_size, stride=1, padding=0, bias=True),
                                         gate, nn.Conv2d(2 * n_pos, 2 * n_pos, kernel_size=1, stride=1, padding=0, bias=True))
        self.sf_conv = nn.Conv2d(dims, dims, kernel_size=1, stride=1, padding=0, bias=False)
        self.register_parameter("agg_weights", nn.Parameter(torch.rand(n_pos, dims, dims)))


class ALIKED(NativeModule):
    _native_prefix = "sp_aliked"
    _native_name = "lightglue_amd.ALIKED: parameter"
    default_conf = ALIKED_DEFAULT_CONF
    required_data_keys = ["image"]
    checkpoint_url = "https://github.com/Shiaoming/ALIKED/raw/main/models/{}.pth"
    n_limit_max = 20000
    cfgs = ALIKED_CFGS

    def __init__(self, conf=None):
        super().__init__()
        self.conf = conf = merge_conf(self.default_conf, conf or {})
        if conf.model_name not in self.cfgs:
            raise ValueError(f"lightglue_amd.ALIKED: unknown model_name {conf.model_name!r}; one of {sorted(self.cfgs)}")
        self._topk = float(conf.detection_threshold) <= 0 and int(conf.max_num_keypoints) > 0
        if conf.force_num_keypoints and not self._topk:
            raise ValueError("lightglue_amd.ALIKED: force_num_keypoints needs detection_threshold <= 0 and "
                             "max_num_keypoints > 0 (aliked.py:648)")
        g = self.cfgs[conf.model_name]
        c1, c2, c3, c4, dim, K, M = g["c1"], g["c2"], g["c3"], g["c4"], g["dim"], g["K"], g["M"]
        self.dim, self.M = dim, M
        self.pool2 = nn.AvgPool2d(kernel_size=2, stride=2)  # aliked.py:656-715
        self.pool4 = nn.AvgPool2d(kernel_size=4, stride=4)
        self.gate = nn.SELU(inplace=True)
        self.block1 = ConvBlock(3, c1, self.gate)
        self.block2 = ResBlock(c1, c2, self.gate, False)
        self.block3 = ResBlock(c2, c3, self.gate, True)
        self.block4 = ResBlock(c3, c4, self.gate, True)
        self.conv1 = nn.Conv2d(c1, dim // 4, 1, bias=False)
        self.conv2 = nn.Conv2d(c2, dim // 4, 1, bias=False)
        self.conv3 = nn.Conv2d(c3, dim // 4, 1, bias=False)
        self.conv4 = nn.Conv2d(dim, dim // 4, 1, bias=False)
        self.score_head = nn.Sequential(nn.Conv2d(dim, 8, 1, bias=False), self.gate,
                                        nn.Conv2d(8, 4, 3, 1, 1, bias=False), self.gate,
                                        nn.Conv2d(4, 4, 3, 1, 1, bias=False), self.gate,
                                        nn.Conv2d(4, 1, 3, 1, 1, bias=False))
        self.desc_head = SDDH(dim, K, M, self.gate)
        if not conf.trainable:
            for p in self.parameters():
                p.requires_grad = False
        self._owners = [m for m in self.modules() if m._parameters or isinstance(m, nn.BatchNorm2d)]
        self._native_init()

    # ------------------------------------------------------------ native handle
    def _native_state(self):
        # bn.num_batches_tracked is an int64 counter the forward does not use
        return {n: t for n, t in self.state_dict(keep_vars=True).items() if not n.endswith("num_batches_tracked")}

    def _weights_signature(self):  # parameters and the BatchNorm running statistics
        sig = []
        for m in self._owners:
            sig += [(id(m), n, t.data_ptr(), t._version) for n, t in m._parameters.items() if t is not None]
            if isinstance(m, nn.BatchNorm2d):
                sig += [(id(m), n, m._buffers[n].data_ptr(), m._buffers[n]._version) for n in ("running_mean", "running_var")]
        return tuple(sig)

    def _create_handle(self, lib, device, h):
        c, g = self.conf, self.cfgs[self.conf.model_name]
        cfg = _lib.AlikedConfig(g["c1"], g["c2"], g["c3"], g["c4"], g["dim"], g["M"], int(c.nms_radius),
                                int(c.max_num_keypoints), float(c.detection_threshold))
        _lib.check(lib.sp_aliked_create(ctypes.byref(cfg), device.index or 0, ctypes.byref(h)), "sp_aliked_create")

    # ------------------------------------------------------------ forward (aliked.py:765-783)
    def forward(self, data: dict) -> dict:
        for k in self.required_data_keys:
            assert k in data, f"Missing key {k} in data"
        c = self.conf
        image = data["image"]
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError(f"image must be [B, 3, H, W], got {tuple(image.shape)}")
        if not image.is_cuda:
            raise RuntimeError("lightglue_amd.ALIKED runs on a HIP device; inputs are on the CPU")
        device = image.device
        image = image.float().contiguous()
        B, _, H, W = image.shape
        n_limit = int(c.max_num_keypoints) if int(c.max_num_keypoints) > 0 else self.n_limit_max
        cap = int(c.max_num_keypoints) if self._topk else min(n_limit, H * W)
        lib = self._ensure_handle(device)
        nb = ctypes.c_size_t()
        _lib.check(lib.sp_aliked_workspace_bytes(self._handle, B, H, W, cap, ctypes.byref(nb)), "sp_aliked_workspace_bytes")
        ws = self._workspace_bytes(nb.value, device)
        isz = data.get("image_size")
        isz = None if isz is None else isz.to(device=device, dtype=torch.float32).contiguous()
        score_map = torch.empty((B, 1, H, W), device=device)
        kpts = torch.empty((B, cap, 2), device=device)
        desc = torch.empty((B, cap, self.dim), device=device)
        sampled = torch.empty((B, cap), device=device)
        disp = torch.empty((B, cap), device=device)
        counts = torch.empty((B,), dtype=torch.int32, device=device)
        host_counts = (ctypes.c_int32 * B)()
        inp = _lib.AlikedInputs(B, H, W, _ptr(image), _ptr(isz))
        out = _lib.AlikedOutputs(_ptr(score_map), cap, _ptr(kpts), _ptr(desc), _ptr(sampled), _ptr(disp), _ptr(counts),
                                 ctypes.cast(host_counts, ctypes.c_void_p))
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _lib.check(lib.sp_aliked_forward(self._handle, ctypes.byref(inp), ctypes.byref(out), _ptr(ws), nb.value, stream),
                   "sp_aliked_forward")
        n = list(host_counts)
        pred = {"score_map": score_map}
        if self._topk:  # exactly k per image, nothing read back
            k = cap
        elif data.get("ragged_keypoints"):
            k = max(n) if n else 0  # the library zero-fills the slots past each count
            pred["num_keypoints"] = counts
        else:
            if len(set(n)) > 1:
                raise RuntimeError(f"stack expects each tensor to be equal size, but got keypoint counts {n} "
                                   "(aliked.py:778; use the top-k mode or data['ragged_keypoints'])")
            k = n[0] if n else 0
        # the reference's swapped unpacking (:768 against :240): see the module docstring
        pred.update({"keypoints": kpts[:, :k], "descriptors": desc[:, :k], "keypoint_scores": disp[:, :k],
                     "score_dispersity": sampled[:, :k]})
        if not self._topk and data.get("ragged_keypoints"):
            real = torch.arange(k, device=device)[None] < counts[:, None]
            pred["descriptors"] = torch.where(real[..., None], pred["descriptors"], torch.zeros((), device=device))
        return pred

    def loss(self, pred, data):
        raise NotImplementedError

    def metrics(self, pred, data):
        raise NotImplementedError
