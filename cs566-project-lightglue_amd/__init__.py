"""MI355X-native LightGlue matcher (gfx950 HIP kernels behind a C-ABI library).

Drop-in for ``gluefactory.models.matchers.lightglue.LightGlue``: same config keys, same
state-dict schema, same ``forward(data) -> dict`` contract.  Import through ``lgamd`` (the
directory name is not an identifier)::

    import lgamd
    from lightglue_amd import LightGlue
"""
from .weights import DEFAULT_CONF, state_dict_schema, synthetic_pair, synthetic_state_dict  # noqa: F401


def __getattr__(name):
    # Lazy: importing the package must not require torch-ROCm or the HIP library.
    if name in ("LightGlue", "__main_model__"):
        from .lightglue import LightGlue

        return LightGlue
    if name == "SuperPoint":
        from .superpoint import SuperPoint

        return SuperPoint
    if name == "SuperPointOpen":
        from .superpoint_open import SuperPoint

        return SuperPoint
    if name == "ALIKED":
        from .aliked import ALIKED

        return ALIKED
    if name == "GlueStick":
        from .gluestick import GlueStick

        return GlueStick
    if name in ("WireframeExtractor", "LSD", "lines_to_wireframe", "sample_descriptors_corner_conv"):
        from . import wireframe

        return getattr(wireframe, name)
    if name in ("SuperGlue", "NLLLoss"):
        from . import superglue

        return getattr(superglue, name)
    if name in ("log_optimal_transport", "filter_matches"):
        from . import assignment

        return getattr(assignment, name)
    if name in ("eval_matches", "eval_matches_homography", "eval_matches_epipolar", "eval_homography_dlt"):
        from . import match_eval

        return getattr(match_eval, name)
    if name in ("HomographyEstimator", "PointLineHomographyEstimator", "load_estimator", "eval_homography_robust",
                "ransac_homography", "ransac_homography_lines"):
        from . import robust

        return getattr(robust, name)
    if name in ("RelativePoseEstimator", "eval_relative_pose_robust", "ransac_relpose"):
        from . import relative_pose

        return getattr(relative_pose, name)
    raise AttributeError(name)
