"""lab_1806_vec_db_amd -- MI355X-native distance / top-k engine behind lab-1806-vec-db's index traits.

Only the hot path lives here: csrc/ (hand-written gfx950 HIP kernels + the C ABI, include/vdbhip.h) and
the host-side mirror of the reference's index / VecDB surface.  There is no CPU fallback.
"""
from ._lib import COSINE, L2SQR, VdbError  # noqa: F401
from .index import GpuIndex, RowMask, calc_dist, calc_dist_u8, merge_topk, pack_mask, range_merge, remove_plan  # noqa: F401
from .labels import AllOf, AnyOf, LabelTerm, Not, matches_filter  # noqa: F401
from .vecdb import VecDB  # noqa: F401

__all__ = ["GpuIndex", "RowMask", "LabelTerm", "AnyOf", "AllOf", "Not", "matches_filter", "VecDB", "calc_dist", "calc_dist_u8", "merge_topk", "pack_mask", "range_merge", "remove_plan", "VdbError", "L2SQR", "COSINE"]
