"""import-name alias: `mebt.fvd.fvd` (reference mebt/fvd/fvd.py) -> mebt_amd.fvd (HIP I3D embeddings, float64 statistics)"""
from mebt_amd.fvd import *  # noqa: F401,F403
from mebt_amd.fvd import (MAX_BATCH, FVD_SAMPLE_SIZE, TARGET_RESOLUTION, preprocess, get_fvd_logits, get_logits,  # noqa: F401
                          load_fvd_model, frechet_distance, polynomial_mmd, compute_fvd, trace_sqrt_product, cov)
