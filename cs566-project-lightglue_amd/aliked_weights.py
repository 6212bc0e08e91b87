"""ALIKED (``gluefactory/models/extractors/aliked.py``): config table, state-dict schema and seeded
recipe weights.  numpy only: no torch, no HIP library.

The trained checkpoints are downloads (aliked.py:601,726-730), so tests and benchmarks run on recipe
weights that behave like trained ones where the kernels can go wrong:

* BatchNorm gammas of mixed sign and non-trivial running statistics;
* ``desc_head.agg_weights`` zero-mean (the default ``torch.rand`` init makes every descriptor nearly
  the same vector);
* every convolution He-scaled (std sqrt(2 / fan_in), 2.4 times PyTorch's default init per layer) and
  ``score_gain`` on the score head's last convolution on top: with the default init the score map
  is nearly flat (std 0.003 around 0.5), neighbouring kept scores are then 5e-7 apart and no
  selection is decidable.  The recipe's score maps span about 0.01 .. 0.95 at gain 1; a gain of 3 or
  more saturates the sigmoid and the fp32 and fp64 selections start to differ.
"""
from collections import OrderedDict

import numpy as np

ALIKED_DEFAULT_CONF = {  # aliked.py:592-599 (+ the BaseModel keys, base_model.py:54-59)
    "name": None,
    "trainable": True,
    "freeze_batch_normalization": False,
    "timeit": False,
    "model_name": "aliked-n16",
    "max_num_keypoints": -1,
    "detection_threshold": 0.2,
    "force_num_keypoints": False,
    "pretrained": True,
    "nms_radius": 2,
}

ALIKED_CFGS = {  # aliked.py:605-642
    "aliked-t16": {"c1": 8, "c2": 16, "c3": 32, "c4": 64, "dim": 64, "K": 3, "M": 16},
    "aliked-n16": {"c1": 16, "c2": 32, "c3": 64, "c4": 128, "dim": 128, "K": 3, "M": 16},
    "aliked-n16rot": {"c1": 16, "c2": 32, "c3": 64, "c4": 128, "dim": 128, "K": 3, "M": 16},
    "aliked-n32": {"c1": 16, "c2": 32, "c3": 64, "c4": 128, "dim": 128, "K": 3, "M": 32},
}


def _bn(n, c):
    return [(f"{n}.weight", (c,)), (f"{n}.bias", (c,)), (f"{n}.running_mean", (c,)), (f"{n}.running_var", (c,)),
            (f"{n}.num_batches_tracked", ())]


def aliked_schema(model_name="aliked-n16"):
    """[(name, shape)] of ``ALIKED.state_dict()`` in the reference's order (a module's own parameters
    come before its children's, so ``desc_head.agg_weights`` precedes ``desc_head.offset_conv``)."""
    g = ALIKED_CFGS[model_name]
    c1, c2, c3, c4, dim, M = g["c1"], g["c2"], g["c3"], g["c4"], g["dim"], g["M"]
    out = []

    def block(n, ci, co, dcn, down):
        cin = ci
        for i in (1, 2):
            if dcn:
                out.extend([(f"{n}.conv{i}.offset_conv.weight", (18, cin, 3, 3)), (f"{n}.conv{i}.offset_conv.bias", (18,)),
                            (f"{n}.conv{i}.regular_conv.weight", (co, cin, 3, 3))])
            else:
                out.append((f"{n}.conv{i}.weight", (co, cin, 3, 3)))
            out.extend(_bn(f"{n}.bn{i}", co))
            cin = co
        if down:
            out.extend([(f"{n}.downsample.weight", (co, ci, 1, 1)), (f"{n}.downsample.bias", (co,))])

    block("block1", 3, c1, False, False)
    block("block2", c1, c2, False, True)
    block("block3", c2, c3, True, True)
    block("block4", c3, c4, True, True)
    out += [("conv1.weight", (dim // 4, c1, 1, 1)), ("conv2.weight", (dim // 4, c2, 1, 1)),
            ("conv3.weight", (dim // 4, c3, 1, 1)), ("conv4.weight", (dim // 4, dim, 1, 1)),
            ("score_head.0.weight", (8, dim, 1, 1)), ("score_head.2.weight", (4, 8, 3, 3)),
            ("score_head.4.weight", (4, 4, 3, 3)), ("score_head.6.weight", (1, 4, 3, 3)),
            ("desc_head.agg_weights", (M, dim, dim)),
            ("desc_head.offset_conv.0.weight", (2 * M, dim, 3, 3)), ("desc_head.offset_conv.0.bias", (2 * M,)),
            ("desc_head.offset_conv.2.weight", (2 * M, 2 * M, 1, 1)), ("desc_head.offset_conv.2.bias", (2 * M,)),
            ("desc_head.sf_conv.weight", (dim, dim, 1, 1))]
    return out


def aliked_state_dict(model_name="aliked-n16", seed=0, gamma_sign="mixed", score_gain=1.0, offset_gain=1.0):
    """Seeded recipe weights (see the module docstring).  ``gamma_sign``: "mixed" (about a quarter
    negative), "negative" or "positive".  ``offset_gain`` scales the offset convolutions (at 1 the
    deformable taps and the SDDH sample positions move by a pixel or two)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for name, shape in aliked_schema(model_name):
        if name.endswith("num_batches_tracked"):
            v = np.asarray(1000, np.int64)
        elif name.endswith("running_mean"):
            v = 0.2 * rng.standard_normal(shape)
        elif name.endswith("running_var"):
            v = 0.3 + 1.2 * rng.random(shape)
        elif ".bn" in name and name.endswith(".weight"):
            mag = 0.5 + rng.random(shape)
            sign = {"mixed": np.where(rng.random(shape) < 0.25, -1.0, 1.0), "negative": -1.0, "positive": 1.0}[gamma_sign]
            v = sign * mag
        elif ".bn" in name and name.endswith(".bias"):
            v = 0.1 * rng.standard_normal(shape)
        elif name == "desc_head.agg_weights":
            v = rng.standard_normal(shape) * np.sqrt(1.0 / (shape[0] * shape[1]))
        elif name.endswith(".bias"):
            v = 0.3 * rng.standard_normal(shape) if "offset_conv" in name else 0.05 * rng.standard_normal(shape)
        else:
            fan = int(np.prod(shape[1:]))
            v = rng.standard_normal(shape) * np.sqrt(2.0 / fan)
            if "offset_conv" in name:
                v *= offset_gain
            if name == "score_head.6.weight":
                v *= score_gain
        sd[name] = np.asarray(v, np.float32 if v.dtype != np.int64 else np.int64)
    return sd
