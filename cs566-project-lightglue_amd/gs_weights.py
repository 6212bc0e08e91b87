"""GlueStick configuration, state-dict schema, deterministic recipe weights and a seeded
wireframe-pair generator.

The schema is the reference module tree (``gluefactory/models/matchers/gluestick.py``):

* ``kenc.encoder`` / ``lenc.encoder`` -- ``MLP([3 | 5] + keypoint_encoder + [D])`` (``:484-514``);
* ``gnn.layers.<i>.update.attn.{proj.0-2, merge}`` and ``gnn.layers.<i>.update.mlp`` -- the
  SuperGlue ``AttentionalPropagation`` inside a ``GNNLayer`` (``:525-579``);
* ``gnn.line_layers.<i>.mlp`` -- ``MLP([3D, 2D, D])`` of ``LineLayer`` (``:582-604``), one per two
  GNN layers;
* ``final_proj``, ``final_line_proj`` (Conv1d(D, D, 1)) and the scalars ``bin_score``,
  ``line_bin_score``.

The recipe draws weights as :mod:`~lightglue_amd.sg_weights` does (NumPy PCG64, host only,
BatchNorm statistics away from the identity) and ``sharpen`` scales the residual branches down and
the two final projections up, so descriptors stay distinctive through the random layers and the
double softmax keeps confident matches.

:func:`wireframe_pair` makes a pair of views of one random wireframe: keypoints are
``[junction slots | other points]``, lines join two distinct junctions (no junction pair twice), and
view 1 is a permutation of view 0's junctions, points and lines with descriptor noise and half of
the lines' endpoints flipped; each view may carry extra junctions, points and lines of its own and
padding junction slots no line touches.
"""
from collections import OrderedDict

import numpy as np

from .sg_weights import _mlp

GS_DEFAULT_CONF = {
    "input_dim": 256,
    "descriptor_dim": 256,
    "weights": None,
    "version": "v0.1_arxiv",
    "keypoint_encoder": [32, 64, 128, 256],
    "GNN_layers": ["self", "cross"] * 9,
    "num_line_iterations": 1,
    "line_attention": False,
    "filter_threshold": 0.2,
    "checkpointed": False,
    "skip_init": False,
    "inter_supervision": None,
    "loss": {"nll_weight": 1.0, "nll_balancing": 0.5, "inter_supervision": [0.3, 0.6]},
}


def merged_conf(conf=None):
    c = dict(GS_DEFAULT_CONF)
    for k, v in (conf or {}).items():
        if k == "loss":
            c["loss"] = {**GS_DEFAULT_CONF["loss"], **(v or {})}
        else:
            c[k] = v
    c["keypoint_encoder"] = list(c["keypoint_encoder"])
    c["GNN_layers"] = list(c["GNN_layers"])
    return c


def gluestick_schema(conf=None):
    """[(name, shape, kind)] in the reference's state-dict order."""
    c = merged_conf(conf)
    d = c["descriptor_dim"]
    out = [("bin_score", (), "scalar"), ("line_bin_score", (), "scalar")]
    out += _mlp("kenc.encoder", [3] + c["keypoint_encoder"] + [d])
    out += _mlp("lenc.encoder", [5] + c["keypoint_encoder"] + [d])
    for i in range(len(c["GNN_layers"])):
        p = f"gnn.layers.{i}.update"
        out += [(f"{p}.attn.merge.weight", (d, d, 1), "conv_w"), (f"{p}.attn.merge.bias", (d,), "conv_b")]
        for j in range(3):
            out += [(f"{p}.attn.proj.{j}.weight", (d, d, 1), "conv_w"), (f"{p}.attn.proj.{j}.bias", (d,), "conv_b")]
        out += _mlp(f"{p}.mlp", [2 * d, 2 * d, d])
    for i in range(len(c["GNN_layers"]) // 2):
        out += _mlp(f"gnn.line_layers.{i}.mlp", [3 * d, 2 * d, d])
    for n in ("final_proj", "final_line_proj"):
        out += [(f"{n}.weight", (d, d, 1), "conv_w"), (f"{n}.bias", (d,), "conv_b")]
    return out


def gluestick_state_dict(conf=None, seed=0, sharpen=True, proj_gain=6.0, line_gain=0.5):
    """Deterministic weights keyed like the reference state dict (float32; the BatchNorm counters
    int64).  ``sharpen``: GNN ``mlp.3`` x 0.05, the encoders' last layer x 0.1, the line layers'
    ``mlp.3`` x ``line_gain`` (large enough that skipping a line layer is far outside every test
    bar), ``final_proj`` / ``final_line_proj`` x ``proj_gain``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for name, shape, kind in gluestick_schema(conf):
        if kind == "conv_w":
            v = (rng.random(shape) * 2.0 - 1.0) / np.sqrt(shape[1])
        elif kind == "conv_b":
            v = (rng.random(shape) * 2.0 - 1.0) / np.sqrt(sd[name[: -len("bias")] + "weight"].shape[1])
        elif kind == "bn_w":
            v = 0.5 + rng.random(shape)
        elif kind == "bn_b":
            v = (rng.random(shape) - 0.5) * 0.2
        elif kind == "bn_mean":
            v = rng.standard_normal(shape) * 0.1
        elif kind == "bn_var":
            v = 0.5 + 1.5 * rng.random(shape)
        elif kind == "bn_count":
            sd[name] = np.array(0, np.int64)
            continue
        else:  # bin_score, line_bin_score (gluestick.py:102-105)
            v = np.array(1.0)
        sd[name] = np.asarray(v, np.float32)
    if sharpen:
        last = 3 * len(merged_conf(conf)["keypoint_encoder"])
        for name in sd:
            if name.startswith("gnn.layers.") and ".mlp.3." in name:
                sd[name] = (sd[name] * 0.05).astype(np.float32)
            if name.startswith("gnn.line_layers.") and ".mlp.3." in name:
                sd[name] = (sd[name] * line_gain).astype(np.float32)
            if name.startswith((f"kenc.encoder.{last}.", f"lenc.encoder.{last}.")):
                sd[name] = (sd[name] * 0.1).astype(np.float32)
            if name.startswith(("final_proj.", "final_line_proj.")):
                sd[name] = (sd[name] * proj_gain).astype(np.float32)
    return sd


def _wire_lines(rng, n_junc, n_lines):
    """``n_lines`` distinct unordered pairs of distinct junctions in [0, n_junc): a hub of degree
    >= 5 at junction 0, then as many untouched junctions as possible in pairs, then random pairs."""
    assert n_junc >= 2 and n_lines <= n_junc * (n_junc - 1) // 2
    pairs, seen = [], set()

    def add(a, b):
        key = (min(a, b), max(a, b))
        if a == b or key in seen or len(pairs) >= n_lines:
            return
        seen.add(key)
        pairs.append((a, b))

    for j in range(1, min(n_junc, 6)):
        add(0, j)
    for j in range(6, n_junc - 1, 2):
        add(j, j + 1)
    while len(pairs) < n_lines:
        a, b = rng.integers(0, n_junc, 2)
        add(int(a), int(b))
    return np.asarray(pairs, np.int64).reshape(-1, 2)


def wireframe_pair(B, junc, pts, lines, seed=0, pad_junc=(0, 0), noise=0.05, width=640, height=480, dim=256):
    """A seeded pair of wireframe views.  ``junc`` / ``pts`` / ``lines``: (view 0, view 1) counts of
    true junctions, other points and lines; the smaller count of each is shared between the views
    (view 1's copies permuted, descriptors noised, every second shared line flipped), the rest is
    the view's own.  ``pad_junc`` junction slots per view follow the true junctions and belong to
    no line.  Returns float32 / int64 arrays keyed like the matcher's inputs (``keypoints*``,
    ``descriptors*``, ``keypoint_scores*``, ``lines*``, ``lines_junc_idx*``, ``line_scores*``) and
    the ground truth (``gt_matches*``, ``gt_assignment``, ``gt_line_matches*``,
    ``gt_line_assignment``)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    (J0, J1), (P0, P1), (L0, L1) = junc, pts, lines
    Jc, Pc, Lc = min(J0, J1), min(P0, P1), min(L0, L1)
    S0, S1 = J0 + pad_junc[0], J1 + pad_junc[1]  # junction slots
    M, N = S0 + P0, S1 + P1
    size = np.array([width, height], np.float64)

    def unit(x):
        return x / np.linalg.norm(x, axis=-1, keepdims=True)

    out = {k: [] for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "keypoint_scores0",
                           "keypoint_scores1", "lines0", "lines1", "lines_junc_idx0", "lines_junc_idx1", "line_scores0",
                           "line_scores1", "gt_matches0", "gt_matches1", "gt_assignment", "gt_line_matches0",
                           "gt_line_matches1", "gt_line_assignment")}
    for _ in range(B):
        # view 0: its own layout [junctions | padding slots | points]
        k0 = rng.random((M, 2)) * (size - 1)
        d0 = unit(rng.standard_normal((M, dim)))
        s0 = rng.random(M)
        # shared lines live on the shared junctions, the view's own lines anywhere on its junctions
        shared = _wire_lines(rng, Jc, Lc) if Lc else np.zeros((0, 2), np.int64)

        def own_lines(J, L, base):
            have = {(min(a, b), max(a, b)) for a, b in base}
            extra = []
            while len(base) + len(extra) < L:
                a, b = (int(v) for v in rng.integers(0, J, 2))
                key = (min(a, b), max(a, b))
                if a != b and key not in have:
                    have.add(key)
                    extra.append((a, b))
            return np.concatenate([base, np.asarray(extra, np.int64).reshape(-1, 2)], 0)

        l0 = own_lines(J0, L0, shared)
        # view 1: shared junctions / points permuted into its own slots
        pj = rng.permutation(J1)[:Jc]          # view-0 junction j -> view-1 junction pj[j]
        pp = S1 + rng.permutation(P1)[:Pc]     # view-0 point S0 + i -> view-1 keypoint pp[i]
        k1 = rng.random((N, 2)) * (size - 1)
        d1 = unit(rng.standard_normal((N, dim)))
        s1 = rng.random(N)
        m0 = -np.ones(M, np.int64)
        m0[:Jc] = pj
        m0[S0:S0 + Pc] = pp
        src = np.nonzero(m0 >= 0)[0]
        k1[m0[src]] = np.clip(k0[src] + rng.standard_normal((len(src), 2)) * 2.0, 0, size - 1)
        d1[m0[src]] = unit(d0[src] + noise * rng.standard_normal((len(src), dim)))
        m1 = -np.ones(N, np.int64)
        m1[m0[src]] = src
        mapped = pj[shared] if Lc else shared
        mapped[1::2] = mapped[1::2, ::-1]      # half of the shared lines flipped
        l1 = own_lines(J1, L1, mapped)
        pl = rng.permutation(L1)               # view-1 line order
        l1p = np.empty_like(l1)
        l1p[pl] = l1
        lm0 = -np.ones(L0, np.int64)
        lm0[:Lc] = pl[:Lc]
        lm1 = -np.ones(L1, np.int64)
        lm1[pl[:Lc]] = np.arange(Lc)
        ga = np.zeros((M, N), bool)
        ga[src, m0[src]] = True
        gla = np.zeros((L0, L1), bool)
        gla[np.arange(Lc), lm0[:Lc]] = True
        for key, v in (("keypoints0", k0), ("keypoints1", k1), ("descriptors0", d0), ("descriptors1", d1),
                       ("keypoint_scores0", s0), ("keypoint_scores1", s1), ("lines0", k0[l0]), ("lines1", k1[l1p]),
                       ("lines_junc_idx0", l0), ("lines_junc_idx1", l1p), ("line_scores0", rng.random(L0)),
                       ("line_scores1", rng.random(L1)), ("gt_matches0", m0), ("gt_matches1", m1), ("gt_assignment", ga),
                       ("gt_line_matches0", lm0), ("gt_line_matches1", lm1), ("gt_line_assignment", gla)):
            out[key].append(v)
    res = {}
    for k, v in out.items():
        a = np.stack(v)
        res[k] = a if a.dtype in (np.int64, np.bool_) else a.astype(np.float32)
    return res


def wireframe_inputs(B, lines, keypoints, seed=0, max_num_lines=None, dim=256, nms_radius=3, width=160, height=120, s=8):
    """Seeded inputs of the wireframe step (``lightglue_amd.wireframe``): per image ``lines[b]`` segments
    (zero-padded to ``max_num_lines`` when given, ``valid_lines`` False there), ``keypoints`` points with
    scores and unit descriptors, and a dense descriptor map [B, dim, height / s, width / s].

    Endpoints sit in tight groups around well-separated sites (members < 0.8 r apart, sites > 1.7 r), so
    many merge; a strip at the top holds a chain of four endpoints 0.9 r apart (one cluster wider than
    2 r), two integer endpoints exactly r apart (they merge: ``<=``) and a keypoint exactly r from an
    integer endpoint (it stays: ``<``).  About a quarter of the keypoints lie within 0.6 r of an
    endpoint.  Every other endpoint-endpoint and keypoint-endpoint distance is outside +-1e-3 of r
    (the draw repeats until it is); ``exact_pairs`` lists the deliberate ones as
    (image, kind, index, endpoint index), kind 0 an endpoint pair and 1 a keypoint."""
    r = float(nms_radius)
    rng = np.random.Generator(np.random.PCG64(seed))
    K = int(keypoints)
    Lcap = max(lines) if max_num_lines is None else int(max_num_lines)
    assert max(lines) <= Lcap and min(lines) >= 4 and (max_num_lines is not None or len(set(lines)) == 1)
    out = {k: [] for k in ("lines", "line_scores", "valid_lines", "keypoints", "keypoint_scores")}
    exact = []
    for b in range(B):
        L = lines[b]
        E = 2 * L
        while True:
            special = [(12 + 0.9 * r * i, 12.0) for i in range(4)] + [(60.0, 12.0), (60.0 + r, 12.0), (90.0, 12.0)]
            n_rand = E - len(special)
            n_sites = max(1, int(0.55 * n_rand))
            sites = []
            while len(sites) < n_sites:
                c = rng.random(2) * np.array([width - 17, height - 48]) + np.array([8, 40])
                if all(np.hypot(*(c - q)) >= 2.5 * r for q in sites):
                    sites.append(c)
            sites = np.asarray(sites)
            which = np.concatenate([np.arange(n_sites), rng.integers(0, n_sites, n_rand - n_sites)])
            ang, rad = rng.random(n_rand) * 2 * np.pi, rng.random(n_rand) * 0.4 * r
            pts = sites[which] + np.stack([np.cos(ang), np.sin(ang)], 1) * rad[:, None]
            ep = np.concatenate([np.asarray(special), pts]).astype(np.float32)
            perm = rng.permutation(E)
            ep = ep[perm]
            where = np.argsort(perm)  # special point i is endpoint where[i]
            kp = (rng.random((K, 2)) * np.array([width - 17, height - 17]) + 8).astype(np.float32)
            near = rng.permutation(K)[: K // 4]
            a2, r2 = rng.random(len(near)) * 2 * np.pi, rng.random(len(near)) * 0.6 * r
            kp[near] = ep[rng.integers(0, E, len(near))] + (np.stack([np.cos(a2), np.sin(a2)], 1) * r2[:, None]).astype(np.float32)
            kx = int(near[0]) if K else -1  # the keypoint exactly r from the integer endpoint (90, 12)
            if K:
                kp[kx] = (90.0 + 3.0, 12.0 + 4.0) if r == 5 else (90.0, 12.0 + r)
            dee = np.hypot(*(ep[:, None].astype(np.float64) - ep[None].astype(np.float64)).transpose(2, 0, 1))
            dke = np.hypot(*(kp[:, None].astype(np.float64) - ep[None].astype(np.float64)).transpose(2, 0, 1))
            bee, bke = np.abs(dee - r) <= 1e-3, np.abs(dke - r) <= 1e-3
            bee[where[4], where[5]] = bee[where[5], where[4]] = False
            if K:
                bke[kx, where[6]] = False
            if not bee.any() and not bke.any() and dee[where[4], where[5]] == r and (not K or dke[kx, where[6]] == r):
                break
        exact.append((b, 0, int(where[4]), int(where[5])))
        if K:
            exact.append((b, 1, kx, int(where[6])))
        ln = np.zeros((Lcap, 2, 2), np.float32)
        ln[:L] = ep.reshape(L, 2, 2)
        sc = np.zeros(Lcap, np.float32)
        sc[:L] = (0.1 + 0.9 * rng.random(L)).astype(np.float32)
        out["lines"].append(ln)
        out["line_scores"].append(sc)
        out["valid_lines"].append(np.arange(Lcap) < L)
        out["keypoints"].append(kp)
        out["keypoint_scores"].append(rng.random(K).astype(np.float32))
    res = {k: np.stack(v) for k, v in out.items()}
    d = rng.standard_normal((B, K, dim))
    res["descriptors"] = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    res["dense_descriptors"] = rng.standard_normal((B, dim, height // s, width // s)).astype(np.float32)
    res["exact_pairs"] = np.asarray(exact, np.int64).reshape(-1, 4)
    return res
