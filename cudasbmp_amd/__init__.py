"""cudasbmp_amd — MI355X-native KGMT kinodynamic planner (drop-in for nipe1783/cudaSBMP's KGMT).

The hot path (expand -> propagate -> collision-check -> bin -> accept -> insert)
is hand-written HIP for gfx950 in csrc/, exposed through the C ABI in
include/sbmp/sbmp.h (libsbmp.so).  This package is the Python host mirror of
the reference's KGMT interface; it has no CPU fallback.
"""
from ._native import NativeLibraryError, SbmpError, LIB_PATH  # noqa: F401
from .kgmt import KGMT, DeviceBuffer, read_obstacles_csv, device_count, reference_seed_from_time, random_tree  # noqa: F401,E501
from .kgmt_batch import KGMTBatch, batch_pack  # noqa: F401
from .tree_query import goal_radius_threshold, tree_query_batch  # noqa: F401
from .tree_recheck import tree_recheck_batch  # noqa: F401
from .tree_paths import tree_paths_batch, tree_trace_batch  # noqa: F401
from .tree_resample import tree_resample_batch  # noqa: F401
from .tree_extract import tree_extract_batch, tree_extract_info  # noqa: F401
from .tree_adopt import tree_adopt_tables  # noqa: F401
from .tree_reanchor import tree_reanchor_batch  # noqa: F401
from .fold import fold_r2_batch, fold_r2_info  # noqa: F401
from .config import load_system_config, DEMO_INITIAL, DEMO_GOAL  # noqa: F401

__all__ = ["KGMT", "KGMTBatch", "batch_pack", "goal_radius_threshold", "tree_query_batch", "tree_recheck_batch", "tree_paths_batch", "tree_trace_batch", "tree_resample_batch", "tree_extract_batch", "tree_extract_info", "tree_adopt_tables", "tree_reanchor_batch", "fold_r2_batch", "fold_r2_info", "DeviceBuffer", "read_obstacles_csv", "device_count", "reference_seed_from_time", "random_tree",
           "load_system_config", "DEMO_INITIAL", "DEMO_GOAL", "NativeLibraryError", "SbmpError", "LIB_PATH"]
