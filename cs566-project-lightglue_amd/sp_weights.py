"""SuperPoint state-dict schema, default config and deterministic recipes (the nonfree model first,
the open model of ``extractors/superpoint_open.py`` at the end of the file).

Schema: the ``nn.Conv2d`` modules that ``gluefactory_nonfree.superpoint.SuperPoint`` registers, in
registration order (reference ``superpoint.py:174-196``): the shared encoder ``conv1a .. conv4b``,
the detector head ``convPa`` / ``convPb`` (when ``has_detector``) and the descriptor head
``convDa`` / ``convDb`` (when ``has_descriptor``).

Recipes (tests, smoke and bench only; the product never calls them): the trained weights are a
network download (``superpoint.py:172,199``) and unavailable here, so

* :func:`superpoint_state_dict` draws He-scaled normal weights and small biases from a NumPy PCG64
  stream (the encoder then keeps O(1) activations through its ten convolutions), and
* :func:`synthetic_images` draws smooth images in [0, 1] (sums of random Gaussian blobs and
  sinusoids), so the detector sees structure rather than white noise.
"""
from collections import OrderedDict

import numpy as np

SP_DEFAULT_CONF = {  # superpoint.py:153-169 (+ the BaseModel keys, base_model.py:54-59)
    "name": None,
    "trainable": True,
    "freeze_batch_normalization": False,
    "timeit": False,
    "has_detector": True,
    "has_descriptor": True,
    "descriptor_dim": 256,
    "sparse_outputs": True,
    "dense_outputs": False,
    "nms_radius": 4,
    "refinement_radius": 0,
    "detection_threshold": 0.005,
    "max_num_keypoints": -1,
    "max_num_keypoints_val": None,
    "force_num_keypoints": False,
    "randomize_keypoints_training": False,
    "remove_borders": 4,
    "legacy_sampling": True,
}

_ENCODER = [("conv1a", 1, 64), ("conv1b", 64, 64), ("conv2a", 64, 64), ("conv2b", 64, 64),
            ("conv3a", 64, 128), ("conv3b", 128, 128), ("conv4a", 128, 128), ("conv4b", 128, 128)]


def superpoint_schema(conf=None):
    """[(name, shape)] in registration order (superpoint.py:179-196)."""
    c = dict(SP_DEFAULT_CONF, **(conf or {}))
    layers = [(n, ci, co, 3) for n, ci, co in _ENCODER]
    if c["has_detector"]:
        layers += [("convPa", 128, 256, 3), ("convPb", 256, 65, 1)]
    if c["has_descriptor"]:
        layers += [("convDa", 128, 256, 3), ("convDb", 256, int(c["descriptor_dim"]), 1)]
    out = []
    for n, ci, co, k in layers:
        out += [(f"{n}.weight", (co, ci, k, k)), (f"{n}.bias", (co,))]
    return out


def superpoint_state_dict(conf=None, seed=0, bias_scale=0.05):
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for name, shape in superpoint_schema(conf):
        if name.endswith(".weight"):
            fan = shape[1] * shape[2] * shape[3]
            v = rng.standard_normal(shape) * np.sqrt(2.0 / fan)
        else:
            v = rng.standard_normal(shape) * bias_scale
        sd[name] = v.astype(np.float32)
    return sd


def synthetic_images(B, C, H, W, seed=0, blobs=24):
    """[B, C, H, W] float32 in [0, 1]: Gaussian blobs + two sinusoids + a little noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((B, C, H, W), np.float64)
    for b in range(B):
        for c in range(C):
            img = np.zeros((H, W))
            for _ in range(blobs):
                cy, cx = rng.random() * H, rng.random() * W
                s = 2.0 + rng.random() * 0.08 * max(H, W)
                img += (rng.random() * 2 - 1) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            f = rng.random(4) * 0.3
            img += 0.3 * np.sin(f[0] * xx + f[1] * yy) * np.cos(f[2] * xx - f[3] * yy)
            img += rng.standard_normal((H, W)) * 0.02
            img -= img.min()
            out[b, c] = img / max(img.max(), 1e-9)
    return out.astype(np.float32)


# ---- the open (MIT) SuperPoint: gluefactory/models/extractors/superpoint_open.py ---------------
SPO_DEFAULT_CONF = {  # superpoint_open.py:77-87 (+ the BaseModel keys, base_model.py:54-59)
    "name": None,
    "trainable": True,
    "freeze_batch_normalization": False,
    "timeit": False,
    "descriptor_dim": 256,
    "nms_radius": 4,
    "max_num_keypoints": None,
    "force_num_keypoints": False,
    "detection_threshold": 0.005,
    "remove_borders": 4,
    "channels": [64, 64, 128, 128, 256],
    "dense_outputs": None,
}

# the twelve VGGBlocks (superpoint_open.py:91-112) in registration order: (module path, c_in, c_out, k)
SPO_BLOCKS = [("backbone.0.0", 1, 64, 3), ("backbone.0.1", 64, 64, 3), ("backbone.1.0", 64, 64, 3),
              ("backbone.1.1", 64, 64, 3), ("backbone.2.0", 64, 128, 3), ("backbone.2.1", 128, 128, 3),
              ("backbone.3.0", 128, 128, 3), ("backbone.3.1", 128, 128, 3), ("detector.0", 128, 256, 3),
              ("detector.1", 256, 65, 1), ("descriptor.0", 128, 256, 3), ("descriptor.1", 256, 256, 1)]
SPO_POOLED = ("backbone.0.1", "backbone.1.1", "backbone.2.1")  # blocks followed by the 2x2 max-pool


def superpoint_open_schema():
    """[(name, shape)] of ``SuperPoint.state_dict()`` in registration order: 12 blocks x
    {conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
    bn.num_batches_tracked} = 84 tensors (``num_batches_tracked`` is an int64 scalar)."""
    out = []
    for n, ci, co, k in SPO_BLOCKS:
        out += [(f"{n}.conv.weight", (co, ci, k, k)), (f"{n}.conv.bias", (co,)), (f"{n}.bn.weight", (co,)),
                (f"{n}.bn.bias", (co,)), (f"{n}.bn.running_mean", (co,)), (f"{n}.bn.running_var", (co,)),
                (f"{n}.bn.num_batches_tracked", ())]
    return out


def superpoint_open_state_dict(seed=0, bias_scale=0.05):
    """Recipe weights of the open model (the trained ``superpoint_v6_from_tf.pth`` is a download):
    He-scaled convolutions and small biases as above; BatchNorm like a trained one -- gamma of
    magnitude 0.5 .. 1.5 with about a quarter of the channels NEGATIVE (the case a max-only pool
    epilogue gets wrong), beta ~ 0.1 N(0, 1), running mean around 0.4 (a post-ReLU mean), running
    variance in [0.3, 1.5]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for n, ci, co, k in SPO_BLOCKS:
        sd[f"{n}.conv.weight"] = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32)
        sd[f"{n}.conv.bias"] = (rng.standard_normal(co) * bias_scale).astype(np.float32)
        sign = np.where(rng.random(co) < 0.25, -1.0, 1.0)
        sd[f"{n}.bn.weight"] = (sign * (0.5 + rng.random(co))).astype(np.float32)
        sd[f"{n}.bn.bias"] = (0.1 * rng.standard_normal(co)).astype(np.float32)
        sd[f"{n}.bn.running_mean"] = (0.4 + 0.1 * rng.standard_normal(co)).astype(np.float32)
        sd[f"{n}.bn.running_var"] = (0.3 + 1.2 * rng.random(co)).astype(np.float32)
        sd[f"{n}.bn.num_batches_tracked"] = np.asarray(1000, np.int64)
    return sd
