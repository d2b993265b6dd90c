"""Drop-in mirrors of the reference's ``src/features`` extractors (same names and signatures), and
``extract_all``: every feature set of a batch from one pack and one engine call."""
from ._frame import extract_all, gp1d_grid, gp1d_points, gp_grid, gp_points  # noqa: F401
from ..augment import (AugmentPlan, GpResamplePlan, RecipePlan, augment_and_extract, boone_augment_and_extract,  # noqa: F401
                       gp_augment_and_extract, plasticc_augment_and_extract)
from .advanced_features import extract_advanced_features  # noqa: F401
from .cesium_features import extract_cesium_features  # noqa: F401
from .fourier_features import extract_fourier_features  # noqa: F401
