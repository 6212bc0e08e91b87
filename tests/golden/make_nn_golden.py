#!/usr/bin/env python3
"""Generate the nearest-neighbour matcher fixtures by running the REAL reference.

Run from the repo root where the reference checkout exists (it does not on the GPU box)::

    python tests/golden/make_nn_golden.py

Imports the reference's ``gluefactory/models/matchers/nearest_neighbor_matcher.py`` (``find_nn``,
``mutual_check``, ``NearestNeighborMatcher`` on the real ``BaseModel``) through synthetic
``gluefactory`` package objects whose ``__path__`` points into the reference (their ``__init__``
files are skipped) and an ``omegaconf`` stand-in (attribute dicts), as the other generators do.

Inputs come from NumPy PCG64 recipes (:func:`recipe`): Gaussian descriptors; two thirds of
min(M, N) points of image 1 are copies of image-0 points plus noise of relative norm uniform in
[0, 1.6]; N/16 further image-1 points are near-duplicates (relative noise 0.25) of already matched
ones.  They are rounded to int8 codes (std 8) and stored as those; tests/nn_ref.py:decode turns
them into unit-normalised fp32 descriptors (``q / 64`` without normalisation for the exact fixture,
whose products and sums are then exact in fp32 whatever the order).

Stored per fixture: the codes; per flavour (nn_ref.FLAVOURS) the reference's fp32 ``matches0/1``
(scores are ``(m > -1)`` -- asserted here) and the undecidable masks of tests/nn_ref.py:margins
under ``tol = 4 max(e, 2.4e-7 S)`` (``e`` the reference's own max |fp32 - fp64| similarity error,
``S`` = max sum_k |a_k b_k|); the dense ``similarity`` / ``log_assignment`` for the exact fixture
only.  The ragged fixture's expected outputs are the reference run per pair on the sliced inputs.
Asserted here (change a failing seed, not the cap): undecidable rows + columns <= 3 % per fixture
and flavour, and the reference's own fp32 and fp64 runs agree on every decidable item.
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nn_ref  # noqa: E402


class _ADict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def _merge(*cfgs):
    out = _ADict()
    for c in cfgs:
        for k, v in (c or {}).items():
            out[k] = _merge(out.get(k) if isinstance(out.get(k), dict) else {}, v) if isinstance(v, dict) else v
    return out


def install_shim():
    om = types.ModuleType("omegaconf")

    class OmegaConf:
        merge = staticmethod(_merge)
        create = staticmethod(lambda d=None: _merge(d or {}))
        set_struct = staticmethod(lambda *a, **k: None)
        set_readonly = staticmethod(lambda *a, **k: None)

    om.OmegaConf = OmegaConf
    om.DictConfig = _ADict
    sys.modules["omegaconf"] = om
    for name, path in [("gluefactory", "gluefactory"), ("gluefactory.models", "gluefactory/models"),
                       ("gluefactory.models.matchers", "gluefactory/models/matchers"),
                       ("gluefactory.models.utils", "gluefactory/models/utils")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    return importlib.import_module("gluefactory.models.matchers.nearest_neighbor_matcher")


def recipe(seed, B, M, N, D):
    """int8 codes q0 [B,M,D], q1 [B,N,D] (module docstring)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x0 = rng.standard_normal((B, M, D))
    x1 = rng.standard_normal((B, N, D))
    nm = (2 * min(M, N)) // 3
    nd = N // 16
    for b in range(B):
        src = rng.permutation(M)[:nm]
        dst = rng.permutation(N)
        noise = rng.standard_normal((nm, D)) * (rng.uniform(0.0, 1.6, (nm, 1)) / np.sqrt(D)) * np.linalg.norm(
            x0[b, src], axis=-1, keepdims=True)
        x1[b, dst[:nm]] = x0[b, src] + noise
        dup = dst[nm:nm + nd]
        if nm and len(dup):
            of = dst[rng.integers(0, nm, len(dup))]
            x1[b, dup] = x1[b, of] + rng.standard_normal((len(dup), D)) * (0.25 / np.sqrt(D)) * np.linalg.norm(
                x1[b, of], axis=-1, keepdims=True)
    # unit direction times 8 sqrt(D): codes of std 8 whatever the noise added
    q = [np.clip(np.rint(x / np.linalg.norm(x, axis=-1, keepdims=True) * 8.0 * np.sqrt(D)), -127, 127).astype(np.int8)
         for x in (x0, x1)]
    return q[0], q[1]


CASES = [
    # name, seed, B, M, N, D, exact, counts
    ("nn_exact_b3_m64_n48_d64", 31, 3, 64, 48, 64, True, None),
    ("nn_b2_m300_n257_d256", 32, 2, 300, 257, 256, False, None),
    ("nn_b2_m513_n512_d256", 33, 2, 513, 512, 256, False, None),
    ("nn_b1_m37_n1100_d128", 34, 1, 37, 1100, 128, False, None),
    ("nn_b1_m1100_n37_d128", 35, 1, 1100, 37, 128, False, None),
    ("nn_b2_m130_n77_d100", 36, 2, 130, 77, 100, False, None),
    ("nn_ragged_b3_m300_n257_d256", 37, 3, 300, 257, 256, False, ([300, 17, 1], [257, 200, 5])),
]


def run_reference(mod, d0, d1, ratio, dist, mutual, counts):
    """The reference's outputs as tensors; a ragged batch pair by pair on the sliced inputs."""
    net = mod.NearestNeighborMatcher({"ratio_thresh": ratio, "distance_thresh": dist, "mutual_check": mutual})
    if counts is None:
        return net({"descriptors0": d0, "descriptors1": d1})
    B, M = d0.shape[:2]
    N = d1.shape[1]
    m0 = torch.full((B, M), -1, dtype=torch.int64)
    m1 = torch.full((B, N), -1, dtype=torch.int64)
    for b in range(B):
        a, c = counts[0][b], counts[1][b]
        if ratio and min(a, c) < 2:
            # no second neighbour on one side (the reference's topk(2) fails): that side has no matches, by
            # this project's rule; the other side and the mutual check are the reference's functions
            sim = torch.einsum("bnd,bmd->bnm", d0[b:b + 1, :a], d1[b:b + 1, :c])
            r0 = mod.find_nn(sim, ratio, dist) if c >= 2 else m0.new_full((1, a), -1)
            r1 = mod.find_nn(sim.transpose(1, 2), ratio, dist) if a >= 2 else m1.new_full((1, c), -1)
            if mutual:
                r0, r1 = mod.mutual_check(r0, r1)
            m0[b, :a], m1[b, :c] = r0[0], r1[0]
            continue
        r = net({"descriptors0": d0[b:b + 1, :a], "descriptors1": d1[b:b + 1, :c]})
        m0[b, :a], m1[b, :c] = r["matches0"][0], r["matches1"][0]
    return {"matches0": m0, "matches1": m1, "matching_scores0": (m0 > -1).float(), "matching_scores1": (m1 > -1).float()}


def main():
    mod = install_shim()
    os.makedirs(nn_ref.HERE, exist_ok=True)
    for name, seed, B, M, N, D, exact, counts in CASES:
        q0, q1 = recipe(seed, B, M, N, D)
        d0, d1 = torch.from_numpy(nn_ref.decode(q0, exact)), torch.from_numpy(nn_ref.decode(q1, exact))
        full = run_reference(mod, d0, d1, None, None, True, None)
        assert full["similarity"].dtype == torch.float32 and full["matches0"].dtype == torch.int64
        e, S, tol = nn_ref.tol_of(d0, d1, full["similarity"])
        if exact:
            assert e == 0.0, e  # the construction: every product and partial sum is exact in fp32
        out = {"q0": q0, "q1": q1}
        meta = {"B": B, "M": M, "N": N, "D": D, "seed": seed, "exact": exact, "e": e, "S": S, "tol": tol,
                "counts": None if counts is None else [list(counts[0]), list(counts[1])]}
        if exact:
            out["similarity"] = full["similarity"].numpy()
            out["log_assignment"] = full["log_assignment"].numpy()
        worst, kept = 0.0, []
        for ratio, dist, mutual in nn_ref.FLAVOURS:
            k = nn_ref.flavour_key(ratio, dist, mutual)
            r32 = run_reference(mod, d0, d1, ratio, dist, mutual, counts)
            r64 = run_reference(mod, d0.double(), d1.double(), ratio, dist, mutual, counts)
            c0, c1 = (None, None) if counts is None else counts
            mg = nn_ref.margins(d0, d1, ratio, dist, mutual, tol, c0, c1)
            ur, uc = mg["und_rows"], mg["und_cols"]
            frac = (ur.sum() + uc.sum()) / (ur.size + uc.size)
            assert frac <= 0.03, (name, k, frac)
            worst = max(worst, frac)
            for key, ok in (("matches0", ~ur), ("matches1", ~uc)):
                a32, a64 = r32[key].numpy(), r64[key].numpy()
                assert np.array_equal(a32[ok], a64[ok]), (name, k, key)
                assert np.array_equal(r32[key.replace("matches", "matching_scores")].numpy(), (a32 > -1).astype(np.float32))
                assert a32.min() >= -1 and a32.max() < 32767
                out[f"{k}/{key}"] = a32.astype(np.int16)
            out[f"{k}/und_rows"], out[f"{k}/und_cols"] = ur, uc
            kept.append(float((r32["matches0"] > -1).float().mean()))
        out["meta_json"] = np.array(json.dumps(meta))
        path = os.path.join(nn_ref.HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: e {e:.3e} S {S:.3f} tol {tol:.3e} worst undecidable {100 * worst:.2f} % "
              f"kept m0 {min(kept):.2f}..{max(kept):.2f}  ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
